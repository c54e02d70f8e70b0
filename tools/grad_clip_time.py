"""Dev tool: what gradient clipping and the non-finite guard ("Gradient clipping and the non-finite guard") add to the
optimiser tail on one MI355X, written to profiles/grad_clip_time.md.  ``ops.novograd_step`` - norm, moment and update kernels on a
kept workspace, as the fused step calls it - at the parameter counts and tensor tables of cfg2 (asr13x1, 28 classes) and cfg5
(asr13x1, the 4334 classes of the AISHELL vocabulary): without a record, with a record in mode "off", with norm clipping + guard and
with value clipping + guard, all variants built first and timed in alternation in this one process.  The calls are replayed from a
hipGraph, as they run inside the captured step, so the host's enqueue time stays out.
python tools/grad_clip_time.py [OUT.md]
python tools/grad_clip_time.py --trace cfg2|cfg5      eager calls of "no record" and "norm + guard" for a kernel trace
                                                      (rocprofv3 --kernel-trace --stats -- python tools/grad_clip_time.py --trace cfg2)
python tools/grad_clip_time.py --kernels RESULTS.db   the optimiser kernels of such a trace: calls and average us"""
import os
import sqlite3
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.ema_time import CALLS, CONFIGS, REPLAYS, ROUNDS, _graph_of, _timed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = (("no record", None), ("record, off", ("off", 0.0, False)), ("norm + guard", ("norm", 1e-3, True)),
            ("value + guard", ("value", 1e-4, True)))
TRACE_CALLS = 200


def tails(dev, n_class, variants):
    """one callable per variant, each on buffers of its own; the gradient is randn * 1e-3, so norm 1e-3 and value 1e-4 both clip"""
    import torch
    from lightning_asr_amd import ops
    from lightning_asr_amd.engine import NativeModel
    m = NativeModel("plain", n_class, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
    m.init_parameters(seed=0)
    n, offs = m.n_param, m.param_offsets()
    n_t = offs.numel() - 1
    grads = torch.randn(n, device=dev) * 1e-3
    lr = torch.tensor([1e-3], dtype=torch.float32, device=dev)

    def tail(rec):
        p, mom = m.params.clone(), torch.zeros(n, device=dev)
        v = torch.zeros(n_t, dtype=torch.float32, device=dev)
        ws = ops.novograd_workspace(n_t, n, dev)
        st = ops.clip_state(*rec, device=dev) if rec is not None else None
        return lambda: ops.novograd_step(p, grads, mom, v, offs, lr, 0.8, 0.5, 1e-8, 1e-3, ws=ws, clip_state=st)
    return n, n_t, {name: tail(rec) for name, rec in variants}


def measure(dev, name, n_class, lines):
    n, n_t, fns = tails(dev, n_class, VARIANTS)
    graphs = {k: _graph_of(fn) for k, fn in fns.items()}
    us = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():              # alternate the variants inside every round
            us[k].append(_timed(g.replay, REPLAYS) * 1e3 / CALLS)
    med = {k: statistics.median(v) for k, v in us.items()}
    del graphs
    cells = ["%.2f (%.2f-%.2f)" % (med[k], min(us[k]), max(us[k])) for k, _ in VARIANTS]
    added = ["%+.2f" % (med[k] - med["no record"]) for k, _ in VARIANTS[1:]]
    lines.append("| %s | %d | %d | %s | %s |" % (name, n, n_t, " | ".join(cells), " | ".join(added)))


def trace(dev, cfg):
    import torch
    _, _, fns = tails(dev, dict(CONFIGS)[cfg], (VARIANTS[0], VARIANTS[2]))
    for fn in fns.values():
        for _ in range(TRACE_CALLS):
            fn()
        torch.cuda.synchronize()


def kernels(db):
    c = sqlite3.connect(db)
    print(" | ".join(r[1] for r in c.execute("pragma table_info(top_kernels)")))
    for r in c.execute("select * from top_kernels"):
        if "novograd" in r[0]:
            print(" | ".join(str(x)[:110] for x in r))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        return kernels(sys.argv[2])
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        return trace(dev, sys.argv[2])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "grad_clip_time.md")
    names = [k for k, _ in VARIANTS]
    lines = ["# Gradient clipping and the non-finite guard: measured cost on one MI355X (`python tools/grad_clip_time.py`)", "",
             "The optimiser tail (`ops.novograd_step` on a kept workspace: norm, moment and update kernels) without a clip record, with a "
             "record in mode off, with norm clipping + guard and with value clipping + guard, at the parameter count and tensor table of "
             "each configuration.  %d calls captured into a hipGraph per variant, %d replays per timed window, %d windows, the variants "
             "alternating in one process; median us per call (min-max).  The buffers are swept over and over and sit in the 256 MB "
             "last-level cache, so every column is a lower bound of what the step pays behind a backward that has swept gigabytes; the "
             "differences are what the record adds." % (CALLS, REPLAYS, ROUNDS), "",
             "| config | parameters | tensors | " + " | ".join("%s, us" % k for k in names) + " | "
             + " | ".join("added by %s, us" % k for k in names[1:]) + " |",
             "|" + "---|" * (3 + len(names) + len(names) - 1)]
    for name, n_class in CONFIGS:
        measure(dev, name, n_class, lines)
    lines += ["", "No test gates on time.  `bench.py` never passes a record."]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
