"""Time lasr_ctc_beam_decode (prune launch + search launch) with HIP events at the shapes the decoder serves: the cfg2
validation batch (B=32, T'=501, C=28), cfg5 (B=32, T'=801, C=4334) and 40 s clips (T'=2001, C=28 and 4334), at beam_width
16/64/128 (and 32 for cfg2), cutoff_top_n 40.  Inputs are peaky log-softmaxed normals (one hot class per frame, the blank 60 %
of the time), as CTC outputs are.  Prints one JSON line per shape.

    python tools/beam_time.py [--reps N] [--out FILE] [--dump FILE.npz] [--oracle]

--dump saves every timed case's outputs (tokens, n_tokens, scores), to compare two builds of the library bit for bit: the inputs
are seeded on the device, so both see the same bits.
--oracle also times the f64 Python oracle (tests/helpers/ctc_beam_oracle.py) on the cfg2 batch at beam 32, on the host."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lightning_asr_amd import ops  # noqa: E402

SHAPES = [("cfg2", 32, 501, 28, (16, 32, 64, 128)), ("cfg5", 32, 801, 4334, (16, 64, 128)),
          ("40s_c28", 32, 2001, 28, (16, 64, 128)), ("40s_c4334", 32, 2001, 4334, (16, 64, 128))]


def peaky(B, T, C, seed, device, hot=10.0, sd=2.0, p_blank=0.6):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, T, C, generator=g, device=device) * sd
    hotc = torch.randint(0, C - 1, (B, T), generator=g, device=device)
    hotc = torch.where(torch.rand(B, T, generator=g, device=device) < p_blank, torch.full_like(hotc, C - 1), hotc)
    x.scatter_add_(2, hotc.unsqueeze(-1), torch.full((B, T, 1), hot, device=device))
    return torch.log_softmax(x, -1).contiguous()


def timed(fn, reps):
    """(median ms, min ms, the last call's outputs) of fn over `reps` HIP-event timings after two warm-up calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], out


def dump_case(dump, case, out, names=("tokens", "n_tokens", "scores")):
    """adds a timed case's output tensors to the dict that --dump saves, as host arrays keyed "<case>.<name>\""""
    for name, t in zip(names, out):
        dump["%s.%s" % (case, name)] = t.cpu().numpy()


def save_dump(path, dump):
    """writes dump_case's dict as one compressed .npz"""
    np.savez_compressed(path, **dump)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--oracle", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    lines, dump = [], {}
    for name, B, T, C, widths in SHAPES:
        x = peaky(B, T, C, 1, dev)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        for W in widths:
            ms, ms_min, out = timed(lambda: ops.ctc_beam_decode(x, lens, C - 1, W, 40, 1.0, 1), a.reps)
            dump_case(dump, "%s.w%d" % (name, W), out)
            rec = {"shape": name, "B": B, "T": T, "C": C, "beam_width": W, "cutoff_top_n": 40, "ms_median": round(ms, 3),
                   "ms_min": round(ms_min, 3), "reps": a.reps, "mean_tokens": round(float(out[1].float().mean()), 1)}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.oracle:
        sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
        import ctc_beam_oracle as O
        x = peaky(32, 501, 28, 1, dev).cpu().numpy()
        t0 = time.time()
        O.beam_search_batch(x, None, 27, 32, 40, 1.0, 1)
        rec = {"shape": "cfg2", "B": 32, "T": 501, "C": 28, "beam_width": 32, "cutoff_top_n": 40, "python_oracle_s": round(time.time() - t0, 2)}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if a.dump:
        save_dump(a.dump, dump)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
