"""Dev tool: the four lasr_wave_augment calls profiles/wave_aug_kernel.txt quotes, 10 of each after 3 warm-up calls, meant to run
under `rocprofv3 --kernel-trace --stats` (the kernels' own time) - it also prints event-timed microseconds per call.
32 rows of 160000 samples (10 s at 16 kHz), PCM16 -> PCM16 in place, as the native ingest calls it:
  noise      noise on every row, no reverb
  rir2048    reverb on every row, K = 2048
  rir8192    reverb on every row, K = 8192
  default    the default probabilities: reverb on 0.3 of the rows (K = 2048), noise on 0.5
With `--summarise DIR OUT` it reads the rocpd database a rocprofv3 run left under DIR and writes OUT: per case the FIR kernel's
time and FLOP/s (2 K flops per output sample of a reverberated row) next to the resampler's loop (profiles/resample_kernel.txt).
The cases run one after the other, so the k-th group of 13 launches of a kernel belongs to the k-th case.
With `--train DIR` it writes a synthetic corpus (640 clips of 10 s, 4 noise clips, 8 RIRs of 2048 taps) under DIR and prints the
steps/s of a short `Trainer.fit` (batch 32, bf16, native ingest) with the noise and RIR keys off and on, alternated twice.
python tools/wave_aug_time.py          |   python tools/wave_aug_time.py --summarise DIR profiles/wave_aug_kernel.txt"""
import glob
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, L, REPS, WARM = 32, 160000, 10, 3
CASES = ["noise", "rir2048", "rir8192", "default"]


def params_of(case):
    """(B, 4) parameter words and the FIR's flops of one call"""
    rnd = random.Random(4)
    rows = []
    for _ in range(B):
        rir = {"noise": -1, "rir2048": 0, "rir8192": 1}.get(case, 0 if rnd.random() < 0.3 else -1)
        noise = rnd.randrange(4) if (case == "noise" or (case == "default" and rnd.random() < 0.5)) else -1
        rows.append((rir, noise, rnd.randrange(100000) if noise >= 0 else 0, 1000 if noise >= 0 else 0))
    flops = sum(2.0 * (2048, 8192)[r[0]] * L for r in rows if r[0] >= 0)
    return rows, flops


def run():
    import numpy as np
    import torch
    from lightning_asr_amd import ops
    dev = torch.device("cuda")
    rng = np.random.RandomState(1)

    def rir(K):
        h = rng.standard_normal(K) * np.exp(-np.arange(K) / (K / 7.0))
        h[0], h[K - 1] = 2.0 * np.abs(h).max() + 1.0, 0.05                 # (the last tap is kept: K taps exactly)
        return h.astype(np.float32)
    aug = ops.WaveAugmenter([rir(2048), rir(8192)], [rng.randint(-9000, 9000, 160000 + 977 * i).astype(np.int16) for i in range(4)], dev)
    assert aug.rir_taps == [2048, 8192]
    x0 = torch.from_numpy(rng.randint(-20000, 20000, (B, L)).astype(np.int16)).to(dev)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    for case in CASES:
        rows, flops = params_of(case)
        params = torch.tensor(rows, dtype=torch.int32, device=dev)
        x = x0.clone()
        for _ in range(WARM):
            aug(x, lens, params, out=x)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            aug(x, lens, params, out=x)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / REPS * 1e3
        print("case %s: %.1f us per call (events around %d calls: three kernels each); FIR %.2f GFLOP -> %.1f TFLOP/s over the whole call"
              % (case, us, REPS, flops / 1e9, flops / us / 1e6 if flops else 0.0))


def summarise(root, out_path):
    import sqlite3
    rows = []
    for p in glob.glob(os.path.join(root, "**", "*.db"), recursive=True):
        db = sqlite3.connect(p)
        names = [r[0] for r in db.execute("select name from sqlite_master where type in ('table', 'view')")]
        view = "kernels" if "kernels" in names else None
        if view is None:
            continue
        rows += list(db.execute("select name, start, end from kernels order by start"))
    per = {}
    for name, start, end in rows:
        for key in ("energy_fir_kernel", "gains_kernel", "mix_kernel"):
            if key in name:
                per.setdefault(key, []).append((end - start) / 1e3)
    lines = ["lasr_wave_augment on one MI355X: `rocprofv3 --kernel-trace --stats -- python tools/wave_aug_time.py`, %d x %d PCM16 -> PCM16 in place," % (B, L),
             "%d calls per case (warm-up included), kernel time averaged over each case's calls; FLOP = 2 K per output sample of a" % (REPS + WARM),
             "reverberated row; the resampler's inner loop, for scale: 8.9 TFLOP/s (profiles/resample_kernel.txt).", ""]
    n = REPS + WARM
    for i, case in enumerate(CASES):
        _, flops = params_of(case)
        parts = []
        for key in ("energy_fir_kernel", "gains_kernel", "mix_kernel"):
            t = per.get(key, [])[i * n:(i + 1) * n]
            parts.append((key, sum(t) / len(t) if t else float("nan"), len(t)))
        fir = parts[0][1]
        lines.append("case %s: %s" % (case, ", ".join("%s %.1f us (%d calls)" % p for p in parts)))
        lines.append("  total %.1f us; FIR %.2f GFLOP -> %.1f TFLOP/s in energy_fir_kernel" % (sum(p[1] for p in parts), flops / 1e9, flops / fir / 1e6 if flops else 0.0))
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def train_rate(root):
    import json
    import subprocess
    import wave
    import numpy as np
    import torch
    from lightning_asr_amd.data_module import LibriDataModule
    from lightning_asr_amd.lightning_compat import Trainer, seed_everything
    from lightning_asr_amd.train import LightingModule
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    labels = [c.strip() for c in open(os.path.join(here, "data", "labels.txt"), encoding="utf-8").readlines()]
    data = os.path.join(root, "synth")
    subprocess.run([sys.executable, os.path.join(here, "tools", "make_synth_data.py"), "--out", data, "--n-train", "640", "--n-dev", "32",
                    "--seconds", "10.0"], check=True)
    rng = np.random.RandomState(1)
    mans = {}
    for key, n_files in (("noise", 4), ("rir", 8)):
        mans[key] = os.path.join(root, key + ".json")
        with open(mans[key], "w") as f:
            for i in range(n_files):
                if key == "noise":
                    pcm = rng.randint(-9000, 9000, 160000 + 977 * i)
                else:
                    h = rng.standard_normal(2048) * np.exp(-np.arange(2048) / (2048 / 7.0))
                    h[0], h[2047] = 2.0 * np.abs(h).max() + 1.0, 0.2
                    pcm = np.rint(h / h[0] * 16000)
                path = os.path.join(root, "%s%d.wav" % (key, i))
                with wave.open(path, "wb") as w:
                    w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.astype("<i2").tobytes())   # noqa: E702
                f.write(json.dumps({"audio_filepath": path}) + "\n")
    for rep in range(2):
        for on in (False, True):
            seed_everything(0)
            kw = dict(noise_manifest=mans["noise"], rir_manifest=mans["rir"]) if on else {}
            dm = LibriDataModule([os.path.join(data, "train.json")], os.path.join(data, "dev.json"), os.path.join(data, "dev.json"), labels,
                                 train_bs=32, dev_bs=32, num_worker=6, device="cuda:0", act_dtype=torch.bfloat16, **kw)
            model = LightingModule(learning_rate=1e-2, weight_decay=1e-3, labels=labels, total_epoch=1, drop_rate=0.0, mask=True, use_cer=True,
                                   dtype="bf16", device="cuda:0", warmup_steps=2)
            stamps = []                              # one event per step on the compute stream: the GPU's own timeline
            tr = Trainer(max_epochs=1, default_root_dir=os.path.join(root, "run%d%d" % (rep, on)), device="cuda:0", check_val_every_n_epoch=1,
                         log_every_n_steps=50)
            tr._fused_on_batch = lambda db: (stamps.append(torch.cuda.Event(enable_timing=True)), stamps[-1].record())
            tr.fit(model, dm)
            torch.cuda.synchronize()
            taps = dm.audio_parser.wave_aug.op().rir_taps if on else None
            print("keys %s (pass %d): %d steps, %.2f steps/s over the last %d (device events at batch hand-over; source %s)%s"
                  % ("on " if on else "off", rep, len(stamps), (len(stamps) - 4) / (stamps[3].elapsed_time(stamps[-1]) * 1e-3), len(stamps) - 4,
                     tr.fused.source_kind if tr.fused is not None else "-", "; RIR taps %s" % (taps,) if on else ""), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--train":
        train_rate(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], sys.argv[3])
    else:
        run()
