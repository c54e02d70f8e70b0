"""Dev tool: what gradient accumulation (accumulate_grad_batches = K; DESIGN 4, "Gradient accumulation") costs on one MI355X, written to
profiles/grad_accum_time.md:
  a. lasr_grad_accumulate on the cfg2 gradient (5 044 572 f32: two 20 MB reads, one 20 MB write), event-timed us per call
     (the calls replayed from a hipGraph, as they run inside the captured step);
  b. the graph-replayed cfg2 step (asr13x1, B = 32, 10 s clips, bf16) for K in {1, 2, 4, 8}: ms per MICRO-batch.  A window is
     K - 1 replays of the accumulate-role graph and one of the boundary-role graph; K = 1 is the step as bench.py replays it.
     The graphs read their batch in place (features and step in one replay, no prefetch), the same for every K, so the
     difference to K = 1 is the accumulation alone.  All K are built first and timed in alternation, ROUNDS times, in this one
     process: two boxes differ by more than the effect.
python tools/grad_accum_time.py [OUT.md]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_TBS = 6.29     # the streaming read these boxes achieve (README)
B, L, S = 32, 160000, 100
KS = (1, 2, 4, 8)
ROUNDS = 7
MICRO_PER_ROUND = 160          # a multiple of every K: ~0.3 s of GPU work per timed window


def _timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n          # ms per call


def kernel_time(dev, lines):
    import torch
    from lightning_asr_amd import ops
    from lightning_asr_amd.engine import NativeModel
    m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
    n = m.n_param
    acc, g = torch.zeros(n, device=dev), torch.randn(n, device=dev)
    sched = m.bucket_schedule(2)
    cases = [("whole buffer (lasr_grad_accumulate)", lambda: ops.grad_accumulate(acc, g))]
    for i, (_, ranges) in enumerate(sched):
        cases.append(("bucket %d of 2, %s (lasr_grad_accumulate_ranges)" % (i, ranges), lambda r=ranges: ops.grad_accumulate(acc, g, r)))
    nbytes = 3 * 4 * n
    lines += ["## a. the accumulate kernel on the cfg2 gradient", "",
              "%d f32 elements: %.1f MB to move per call (two reads, one write); at the %.2f TB/s streaming read of these boxes "
              "that is %.1f us.  100 calls captured into a hipGraph, 20 replays per window after 50 warm-up calls, %d windows (the calls run "
              "back to back: the launch boundary between two kernels is inside the figure, the host's enqueue time is not).  "
              "The same 40 MB are added over and over and fit the 256 MB last-level cache, so this is the kernel's lower bound; in "
              "the step, behind a backward that has swept gigabytes, the operands come from HBM: table b has that figure."
              % (n, nbytes / 1e6, STREAM_TBS, nbytes / STREAM_TBS / 1e6, ROUNDS), "",
              "| case | median us | min | max | TB/s at the median |", "|---|---|---|---|---|"]
    for name, fn in cases:
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()          # 100 calls per replay: the host's enqueue rate (~9 us per eager call) stays out
        with torch.cuda.graph(graph):
            for _ in range(100):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        us = [_timed(graph.replay, 20) * 1e3 / 100 for _ in range(ROUNDS)]
        med = statistics.median(us)
        frac = 1.0 if name.startswith("whole") else sum(hi - lo for lo, hi in sched[int(name.split()[1])][1]) / n
        lines.append("| %s | %.2f | %.2f | %.2f | %.2f |" % (name, med, min(us), max(us), nbytes * frac / med / 1e6))
    lines.append("")


def step_time(dev, lines):
    import torch
    import bench
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.schedule import CosineAnnealingWarmupRestarts
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    wave, tg, tl = bench.synth_batch(B, L, S, 1234, dev)
    runs = {}
    for K in KS:
        m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
        m.init_parameters(seed=0)
        sc = CosineAnnealingWarmupRestarts(None, first_cycle_steps=100000, cycle_mult=2, max_lr=1e-3, min_lr=1e-4, warmup_steps=1000, gamma=0.5)
        ts = TrainStep(m, 1e-3, 1e-3, schedule=sc, accumulate=K)
        graphs = {}
        for role in (("boundary",) if K == 1 else ("accumulate", "boundary")):
            g = GraphedTrainStep(ts, B, L, S, prefetch=False, want_logp=False, inputs=(wave, None, tg, tl), role=role)
            g.capture()
            graphs[role] = g

        def window(K=K, graphs=graphs):
            for _ in range(K - 1):
                graphs["accumulate"].replay()
            graphs["boundary"].replay()
        for _ in range(max(1, 16 // K)):
            window()
        torch.cuda.synchronize()
        runs[K] = (window, [])
    for _ in range(ROUNDS):
        for K in KS:                         # alternate the variants inside every round
            window, ms = runs[K]
            ms.append(_timed(window, MICRO_PER_ROUND // K) / K)
    base = statistics.median(runs[1][1])
    lines += ["## b. the graph-replayed cfg2 step, ms per micro-batch", "",
              "asr13x1, B = %d, 10 s clips, bf16, features and step in one replay.  %d micro-batches per timed window, %d windows per "
              "K, the four K alternating." % (B, MICRO_PER_ROUND, ROUNDS), "",
              "| K | median ms / micro-batch | min | max | against K = 1 |", "|---|---|---|---|---|"]
    for K in KS:
        ms = runs[K][1]
        med = statistics.median(ms)
        lines.append("| %d | %.4f | %.4f | %.4f | %+.1f us (%+.2f %%) |" % (K, med, min(ms), max(ms), (med - base) * 1e3, (med / base - 1) * 100))
    lines += ["", "Estimate before the measurement: 60.5 MB at %.2f TB/s = %.1f us, one more launch boundary 1.7-1.9 us, one 20 MB "
              "zeroing per window: about 0.6 %% of a 1.98 ms step.  K > 1 also SAVES the optimiser (three launches, six passes "
              "over 20 MB) on K - 1 of K micro-batches, which is why the per-micro-batch cost can fall below K = 1's."
              % (STREAM_TBS, 60.5e6 / STREAM_TBS / 1e6), ""]


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("grad_accum_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "grad_accum_time.md")
    lines = ["# Gradient accumulation: measured cost on one MI355X (`python tools/grad_accum_time.py`)", ""]
    kernel_time(dev, lines)
    step_time(dev, lines)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
