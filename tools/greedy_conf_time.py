"""Time ops.greedy_confidence against the best composition the library offered before it for the same outputs (torch max over
the classes, ops.greedy_decode, torch segmented sums by scatter), on the MI355X:

    python tools/greedy_conf_time.py --out profiles/greedy_confidence_time.md

Protocol: both forms warmed, then `--repeats` alternating rounds; a round times `--iters` back-to-back calls of one form between
two device events.  Reported per shape: the median round of each form, the spread (min .. max) of the rounds, and the share of
the 6.29 TB/s streaming-read rate (MI355X, float4 copy) that the op's read of the (B, T, C) block reaches over its median time.
The comparison's outputs are checked against the op's once, before anything is timed."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightning_asr_amd import ops  # noqa: E402

HBM_READ_BPS = 6.29e12
SHAPES = [(32, 801, 4334), (32, 501, 28), (32, 2001, 28)]


def composition(logp, lens, blank):
    """the same outputs from what the library had: max over classes, ops.greedy_decode, segmented sums by scatter"""
    B, T, _ = logp.shape
    dev = logp.device
    m, a = logp.max(-1)
    a32 = a.to(torch.int32)
    tokens, n_tokens = ops.greedy_decode(a32, lens, blank)
    t = torch.arange(T, device=dev).unsqueeze(0)
    valid = t < lens.unsqueeze(1)
    prev = torch.cat([torch.full((B, 1), -1, dtype=a32.dtype, device=dev), a32[:, :-1]], 1)
    label = valid & (a32 != blank)
    emit = label & (a32 != prev)
    slot = torch.where(label, torch.cumsum(emit, 1) - 1, T + t)      # a frame of no token goes to a slot of its own: no contention
    m64 = m.double()
    s = torch.zeros(B, 2 * T, dtype=torch.float64, device=dev).scatter_add_(1, slot, m64)
    cnt = torch.zeros(B, 2 * T, dtype=torch.float64, device=dev).scatter_add_(1, slot, torch.ones_like(m64))
    mn = torch.full((B, 2 * T), float("inf"), device=dev).scatter_reduce_(1, slot, m, "amin")
    start = torch.full((B, 2 * T), T, dtype=torch.int64, device=dev).scatter_reduce_(1, slot, t.expand(B, T), "amin")
    end = torch.full((B, 2 * T), -1, dtype=torch.int64, device=dev).scatter_reduce_(1, slot, t.expand(B, T) + 1, "amax")
    live = t < n_tokens.unsqueeze(1)
    tok_mean = torch.where(live, (s[:, :T] / cnt[:, :T].clamp(min=1)).float(), torch.zeros((), device=dev))
    tok_min = torch.where(live, mn[:, :T], torch.zeros((), device=dev))
    tok_start = torch.where(live, start[:, :T], torch.full((), -1, dtype=torch.int64, device=dev)).to(torch.int32)
    tok_end = torch.where(live, end[:, :T], torch.full((), -1, dtype=torch.int64, device=dev)).to(torch.int32)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    utt = torch.stack([torch.where(valid, m64, zero).sum(1), torch.where(label, m64, zero).sum(1)], 1)
    nb = label.sum(1).to(torch.int32)
    cnts = torch.stack([lens.double(), nb.double()], 1)
    conf = (-(-1e-5 + utt) / (cnts + 1e-6)).float()
    return ops.GreedyConfidence(tokens, n_tokens, tok_start, tok_end, tok_mean, tok_min, utt, nb, conf)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_confidence_time.md"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("greedy_conf_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    rows = []
    for B, T, C in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(B + T + C)
        logp = torch.empty(B, T, C, device=dev)
        for b in range(B):                          # (filled per utterance: the host copy of the large shape is 444 MB)
            x = torch.randn(T, C, generator=g) * 2
            x[:, C - 1] += float(torch.tensor(float(C)).log()) + 1.0
            logp[b] = torch.log_softmax(x, -1).to(dev)
        lens = torch.tensor([T - (7 * b) % (T // 4) for b in range(B)], dtype=torch.int32, device=dev)
        blank = C - 1
        new = lambda: ops.greedy_confidence(logp, lens, blank)  # noqa: E731
        old = lambda: composition(logp, lens, blank)  # noqa: E731
        a, b_ = new(), old()
        torch.cuda.synchronize()
        for k in ("tokens", "n_tokens", "tok_start", "tok_end", "tok_min", "n_nonblank"):
            assert torch.equal(getattr(a, k), getattr(b_, k)), (k, (B, T, C))
        assert torch.allclose(a.conf, b_.conf, rtol=1e-6) and torch.allclose(a.tok_mean, b_.tok_mean, rtol=1e-6)
        for _ in range(3):
            timed(new, args.iters), timed(old, args.iters)
        t_new, t_old = [], []
        for _ in range(args.repeats):
            t_new.append(timed(new, args.iters))
            t_old.append(timed(old, args.iters))
        nbytes = int(lens.sum()) * C * 4
        med_new, med_old = statistics.median(t_new), statistics.median(t_old)
        rows.append((B, T, C, nbytes, med_new, min(t_new), max(t_new), med_old, min(t_old), max(t_old)))
        print(rows[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("# ops.greedy_confidence against the composition it replaces (MI355X)\n\n")
        f.write("Written by `tools/greedy_conf_time.py` (%d alternating rounds of %d back-to-back calls between device events, after\n"
                "warm-up; times in microseconds per call: median, and min .. max of the rounds).  Composition: `logp.max(-1)`,\n"
                "`ops.greedy_decode`, torch scatter sums for the spans, means, minima and utterance sums (a frame outside every token\n"
                "scatters to a slot of its own, so no two runs contend for an address).  Bytes: the frames inside\n"
                "`lens` times C times 4 (padding frames are not read); share = bytes / median time / 6.29 TB/s.  Back-to-back\n"
                "calls on the same block: shapes smaller than the 256 MiB Infinity Cache are served from it, and at C = 28 the call is\n"
                "two dependent launches over a few MB, so its time is launch latency and host enqueue, not bandwidth: the share is\n"
                "printed for completeness only.\n\n" % (args.repeats, args.iters))
        f.write("| B, T, C | bytes read | greedy_confidence | composition | ratio | share of 6.29 TB/s |\n|---|---|---|---|---|---|\n")
        for B, T, C, nbytes, mn, lo, hi, mo, lo2, hi2 in rows:
            f.write("| %d, %d, %d | %.1f MB | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.2fx | %.1f %% |\n"
                    % (B, T, C, nbytes / 1e6, mn, lo, hi, mo, lo2, hi2, mo / mn, 100.0 * nbytes / (mn * 1e-6) / HBM_READ_BPS))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
