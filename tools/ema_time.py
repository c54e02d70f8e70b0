"""Dev tool: what the weight EMA (train.ema_decay > 0; DESIGN 4, "Weight EMA") adds to the optimiser tail on one MI355X, written to
profiles/ema_time.md.  ``ops.novograd_step`` - norm, moment and update kernels on a kept workspace, as the fused step calls it - at
the parameter counts and tensor tables of cfg2 (asr13x1, 28 classes) and cfg5 (asr13x1, the 4334 classes of the AISHELL
vocabulary), with and without ``ema``, both variants built first and timed in alternation in this one process (two boxes differ by more than the effect).  The calls are
replayed from a hipGraph, as they run inside the captured step, so the host's enqueue time stays out.  Next to the added
microseconds: the estimate 2 x bytes / 6.29 TB/s (one more read and one more write of the parameter buffer), and the standalone
``ops.ema_update`` on the same buffers.
python tools/ema_time.py [OUT.md]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_TBS = 6.29     # the streaming read these boxes achieve (README)
ROUNDS = 9
CALLS = 50            # calls per captured graph
REPLAYS = 10          # replays per timed window
CONFIGS = (("cfg2", 28), ("cfg5", 4334))


def _timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n          # ms per call


def _graph_of(fn):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CALLS):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def measure(dev, name, n_class, lines):
    import torch
    from lightning_asr_amd import ops
    from lightning_asr_amd.engine import NativeModel
    m = NativeModel("plain", n_class, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
    m.init_parameters(seed=0)
    n, offs = m.n_param, m.param_offsets()
    n_t = offs.numel() - 1
    grads = torch.randn(n, device=dev) * 1e-3
    lr = torch.tensor([1e-3], dtype=torch.float32, device=dev)

    def tail(with_ema):
        p, mom = m.params.clone(), torch.zeros(n, device=dev)
        v = torch.zeros(n_t, dtype=torch.float32, device=dev)
        ws = ops.novograd_workspace(n_t, n, dev)
        ema = p.clone() if with_ema else None
        st = ops.ema_state(0.999, True, 0, device=dev) if with_ema else None
        return lambda: ops.novograd_step(p, grads, mom, v, offs, lr, 0.8, 0.5, 1e-8, 1e-3, ws=ws, ema=ema, ema_state=st)
    e, p2 = m.params.clone(), m.params.clone() + 1e-3
    # the callables own the buffers their graphs address: they stay referenced for as long as the graphs are replayed
    fns = {"off": tail(False), "on": tail(True), "standalone": lambda: ops.ema_update(e, p2, 0.001)}
    graphs = {k: _graph_of(fn) for k, fn in fns.items()}
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():              # alternate the variants inside every round
            us[k].append(_timed(g.replay, REPLAYS) * 1e3 / CALLS)
    med = {k: statistics.median(v) for k, v in us.items()}
    del graphs
    del fns
    est = 2 * 4 * n / STREAM_TBS / 1e6
    lines.append("| %s | %d | %d | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %+.2f | %.2f | %.2f (%.2f-%.2f) |"
                 % (name, n, n_t, med["off"], min(us["off"]), max(us["off"]), med["on"], min(us["on"]), max(us["on"]),
                    med["on"] - med["off"], est, med["standalone"], min(us["standalone"]), max(us["standalone"])))
    return med


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ema_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ema_time.md")
    lines = ["# Weight EMA: measured cost on one MI355X (`python tools/ema_time.py`)", "",
             "The optimiser tail (`ops.novograd_step` on a kept workspace: norm, moment and update kernels) with and without `ema`, at the "
             "parameter count and tensor table of each configuration.  %d calls captured into a hipGraph per variant, %d replays per timed "
             "window, %d windows, the variants alternating in one process; median us per call (min-max).  The buffers (%s) are swept "
             "over and over and sit in the 256 MB last-level cache, so both columns are lower bounds of what the step pays behind a "
             "backward that has swept gigabytes; their difference is what the average adds to the update kernel.  Estimate: one more "
             "read and one more write of the parameter buffer, 2 x 4 B x n at the %.2f TB/s streaming read of these boxes.  "
             "`ema_update`: the standalone kernel on the same two buffers (one more launch, and the parameters read again)."
             % (CALLS, REPLAYS, ROUNDS, "parameters, gradient, momentum, average", STREAM_TBS), "",
             "| config | parameters | tensors | tail without ema, us | tail with ema, us | added us | estimate us | standalone `ema_update`, us |",
             "|---|---|---|---|---|---|---|---|"]
    for name, n_class in CONFIGS:
        measure(dev, name, n_class, lines)
    lines += ["", "No test gates on time.  `bench.py` never turns the average on."]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
