"""Dev tool: the times profiles/long_recordings_time.txt quotes.
  1. ``ops.vad_segments`` (lasr_vad_segment: a memset and two launches) on a synthetic 10-minute and a 60-minute PCM16 recording:
     events around 20 calls after 3 warm-up calls.
  2. ``AsrTranslator.translate_long`` on the 10-minute recording with a formula-weight checkpoint (greedy decoder, timed=True,
     batch_size 32): the host clock around the call, and around its parts with a device synchronise after each - loading the
     file (host decode + upload), segmenting (with the read-back of the count and the table), gathering, and the rest of the
     batches (features, forward, decode, alignment).  One warm-up call, then 3 timed ones.
The recording: a noise floor at 0.001 and bursts of a gliding tone with noise, 1 to 9 s long, 0.35 to 2 s apart, from a seed.
python tools/long_time.py [OUT.txt]      |      rocprofv3 --kernel-trace --stats ... -- python tools/long_time.py --vad-only
(part 1 alone: the split of the call between its two kernels)"""
import os
import sys
import tempfile
import time
import wave as wavmod

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def recording(minutes: float, seed: int):
    """(n,) int16 on the host"""
    import numpy as np
    g = np.random.RandomState(seed)
    n = int(minutes * 60 * 16000)
    y = (0.001 * g.standard_normal(n)).astype(np.float32)
    t = 0
    while t < n:
        t += int(g.uniform(0.35, 2.0) * 16000)
        m = min(int(g.uniform(1.0, 9.0) * 16000), max(n - t, 0))
        if m <= 0:
            break
        k = np.arange(m, dtype=np.float32) / 16000.0
        y[t:t + m] += (0.2 * np.sin(2 * np.pi * (200.0 + 40.0 * k) * k) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * k))).astype(np.float32)
        y[t:t + m] += (0.02 * g.standard_normal(m)).astype(np.float32)
        t += m
    return np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)


def checkpoint(path):
    import torch
    from oracle import ref_cpu as R
    from lightning_asr_amd.predict import EN_LABELS
    state = R.formula_state("plain", 29)
    for k_ in state:
        if k_.endswith("running_var"):
            state[k_] = state[k_] * 0 + 0.5 + 0.01 * torch.arange(state[k_].numel()).float() % 1.0
    torch.save({"state_dict": {"encoder." + k_: v for k_, v in state.items()},
                "hyper_parameters": {"learning_rate": 1e-2, "weight_decay": 1e-3, "labels": EN_LABELS, "total_epoch": 1, "drop_rate": 0.0,
                                     "mask": True, "use_cer": False}, "epoch": 0, "global_step": 0}, path)


def main(out_path, vad_only=False):
    import torch
    from lightning_asr_amd import ops, predict
    dev = torch.device("cuda")
    lines = ["Long recordings on one MI355X (tools/long_time.py).", ""]
    pcm10 = recording(10, 1)
    for minutes, pcm in ((10, pcm10), (60, recording(60, 2))):
        wave = torch.from_numpy(pcm).to(dev)
        for _ in range(3):
            res = ops.vad_segments(wave)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            res = ops.vad_segments(wave)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 20 * 1e3
        lines.append("ops.vad_segments, %d-minute PCM16 recording (%d samples, %d frames): %.1f us per call (events around 20 calls), "
                     "%d segments; the samples are %.1f MB -> %.2f TB/s effective" % (minutes, wave.numel(), -(-wave.numel() // 160), us,
                                                                                     int(res.n_segs), wave.numel() * 2 / 1e6, wave.numel() * 2 / us / 1e6))
        del wave
    if vad_only:
        print("\n".join(lines))
        return
    d = tempfile.mkdtemp()
    wav = os.path.join(d, "rec10.wav")
    with wavmod.open(wav, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000); f.writeframes(pcm10.astype("<i2").tobytes())
    checkpoint(os.path.join(d, "formula.ckpt"))
    tr = predict.AsrTranslator(os.path.join(d, "formula.ckpt"), map_location="cuda")
    parts = {}

    def timed(name, fn):
        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            if name == "segment":
                int(r.n_segs)
            torch.cuda.synchronize()
            parts[name] = parts.get(name, 0.0) + time.perf_counter() - t0
            return r
        return wrapper

    class Ops:                                     # predict's view of ops, with two calls timed
        def __getattr__(self, name):
            return getattr(ops, name)
    shim = Ops()
    shim.vad_segments = timed("segment", ops.vad_segments)
    shim.gather_segments = timed("gather", ops.gather_segments)
    predict.ops = shim
    predict.load_wav = timed("load", predict.load_wav)
    totals = []
    for run in range(4):
        parts.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.translate_long(wav)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        if run:
            totals.append((total, dict(parts)))
    lines += ["", "translate_long, the 10-minute recording as a wav file, formula weights (plain variant), greedy, timed=True, batch_size 32: "
              "%d segments, longest %.2f s; 3 calls after one warm-up call, host clock, a device synchronise after each part:"
              % (len(res["segments"]), max(s["end"] - s["start"] for s in res["segments"]))]
    for total, p in totals:
        rest = total - sum(p.values())
        lines.append("  total %.1f ms = load %.1f (wav decode on the host) + segment %.2f (with the read-back) + gather %.2f + batches %.1f "
                     "(upload, features, forward, decode, align);  segmenting is %.2f %% of the call, gathering %.2f %%"
                     % (total * 1e3, p["load"] * 1e3, p["segment"] * 1e3, p["gather"] * 1e3, rest * 1e3, 100 * p["segment"] / total,
                        100 * p["gather"] / total))
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text)


if __name__ == "__main__":
    if "--vad-only" in sys.argv[1:]:
        main(None, vad_only=True)
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
