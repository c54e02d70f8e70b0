"""Dev tool: what a training step of the "q105" variant (QuartNet105: 52 units against the plain variant's 15) costs on one
MI355X, written to profiles/q105_time.md next to a plain-variant step measured in the same call.  The graph-replayed bf16 step as
bench.py runs it (synthetic batches resident in HBM, the next step's features inside this step's loss launch, two graphs
ping-ponging the feature buffers) at the cfg2 shape (B = 32, 10 s, 28 classes) and at B = 8, then the same step eager with the
library's event brackets for the per-class totals (lasr_prof).

Every measurement is a child process (the library is loaded once per process), the configurations alternating round by round, one
process on the GPU at a time.  ``--parent-lib PATH``: a liblasr.so built from the parent revision; the plain step is then also
measured on it, alternating with this tree's, to show whether this change moved the plain step.

python tools/q105_time.py [--parent-lib PATH] [--out OUT.md] [--rounds N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXPLAIN = ("An inner unit of a block has one 1x1 GEMM and one BatchNorm side where a residual unit of the plain variant has two of each, and the head, the feature kernel and the optimiser are paid once per step whatever the depth: the depthwise class scales with the unit count, the others stay below it.")
NAIVE_PLAIN_MS = 1.98       # the plain step of BENCH (cfg2, bf16); the naive estimate for q105 is 52 / 15 of it


def child(variant, B, windows, steps):
    import torch
    import bench
    from lightning_asr_amd import _lib
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    dev = torch.device("cuda:0")
    m = NativeModel(variant, 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
    m.init_parameters(seed=0)
    ts = TrainStep(m, 1e-2, 1e-3)
    L = 160000
    batches = [bench.synth_batch(B, L, 100, seed, dev, 27) for seed in (1234, 991234)]
    F0, p0 = ts.features(batches[0][0])
    F0, p0 = F0.clone(), p0.clone()
    F1, p1 = torch.empty_like(F0), torch.empty_like(p0)
    graphs = []
    for i in range(2):
        cur, nxt = batches[i], batches[1 - i]
        g = GraphedTrainStep(ts, B, L, cur[1].shape[1], prefetch=True, inputs=(nxt[0], None, cur[1], cur[2]),
                             feats_in=(F0, p0) if i == 0 else (F1, p1), feats_out=(F1, p1) if i == 0 else (F0, p0))
        g.capture()
        graphs.append(g)
    f, p_ = ts.features(batches[0][0])
    F0.copy_(f); p0.copy_(p_)
    n = 0
    for _ in range(6):
        graphs[n % 2].replay(); n += 1
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(steps):
            last = graphs[n % 2].replay(); n += 1
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    loss = float(last[0].item())
    # per-class totals: eager steps through the library's event brackets (a replay does not pass through the launch path)
    lib = _lib.load()
    n_prof = 4
    ts.step(batches[0][0], batches[0][1], batches[0][2], prefetch_wave=batches[1][0], want_logp=False)
    torch.cuda.synchronize()
    lib.lasr_prof_enable(1)
    for i in range(n_prof):
        b, nx = batches[i % 2], batches[1 - i % 2]
        ts.step(b[0], b[1], b[2], prefetch_wave=nx[0], want_logp=False)
    torch.cuda.synchronize()
    lib.lasr_prof_enable(0)
    pms = (C.c_double * 8)(); fl = (C.c_double * 8)(); by = (C.c_double * 8)(); cnt = (C.c_int64 * 8)()
    _lib.check(lib.lasr_prof_collect(pms, fl, by, cnt), "lasr_prof_collect")
    classes = {k: {"ms": pms[i] / n_prof, "brackets": cnt[i] / n_prof} for i, k in enumerate(bench.PROF_KINDS)}
    print(json.dumps({"variant": variant, "B": B, "ms": ms, "loss": loss, "classes": classes, "units": len(m.unit_names()),
                      "workspace_bytes": int(m._ws.numel())}))


def run_child(variant, B, lib_path, windows, steps):
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("LASR_"):
            del env[k]
    if lib_path:
        env["LASR_LIB_PATH"] = lib_path
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant, str(B), str(windows), str(steps)], env=env,
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit("child %s B=%d failed (rc %d):\n%s" % (variant, B, out.returncode, out.stderr[-3000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q105_time.md"))
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("q105_time.py measures on the GPU; none found")
    windows, steps = 3, 20
    res = {}
    for B in (32, 8):
        legs = [("plain", "plain", None), ("q105", "q105", None)]
        if args.parent_lib and B == 32:
            legs.insert(1, ("plain, parent revision", "plain", os.path.abspath(args.parent_lib)))
        for _ in range(args.rounds):
            for label, variant, lib_path in legs:          # the legs alternate inside every round
                r = run_child(variant, B, lib_path, windows, steps)
                e = res.setdefault((B, label), {"ms": [], "classes": r["classes"], "units": r["units"], "ws": r["workspace_bytes"]})
                e["ms"] += r["ms"]
                print("B=%d %-24s %s ms" % (B, label, " ".join("%.3f" % v for v in r["ms"])), flush=True)
    lines = ["# The q105 training step: measured on one MI355X (`python tools/q105_time.py --parent-lib <parent's liblasr.so>`)", "",
             "The graph-replayed bf16 training step as `bench.py` runs it (synthetic 10 s clips resident in HBM, 28 classes, the next "
             "step's features inside the loss launch), %d rounds x %d windows of %d replays per leg, every leg its own process, the legs "
             "alternating round by round; median ms per step (min-max).  Per-class columns: eager steps through the library's event "
             "brackets (`lasr_prof`), ms per step (brackets per step) - their sum exceeds the replayed step by the brackets' own events "
             "and the host's enqueue gaps." % (args.rounds, windows, steps), "",
             "| B | leg | units | step, ms | gemm | dwconv | bn | head | other | workspace, MB |", "|---|---|---|---|---|---|---|---|---|---|"]
    med = {}
    for (B, label), e in res.items():
        med[(B, label)] = statistics.median(e["ms"])
        cl = e["classes"]
        lines.append("| %d | %s | %d | %.3f (%.3f-%.3f) | %s | %.0f |"
                     % (B, label, e["units"], med[(B, label)], min(e["ms"]), max(e["ms"]),
                        " | ".join("%.3f (%.0f)" % (cl[k]["ms"], cl[k]["brackets"]) for k in ("gemm", "dwconv", "bn", "head", "other")),
                        e["ws"] / 1e6))
    lines.append("")
    q, p = med[(32, "q105")], med[(32, "plain")]
    naive = 52.0 / 15.0 * NAIVE_PLAIN_MS
    lines.append("Naive estimate at B = 32: 52 / 15 units x the plain step's %.2f ms = %.2f ms; against the plain step measured here "
                 "(%.3f ms) it is %.3f ms.  Measured: %.3f ms, %+.1f %% against the first and %+.1f %% against the second."
                 % (NAIVE_PLAIN_MS, naive, p, 52.0 / 15.0 * p, q, 100 * (q / naive - 1), 100 * (q / (52.0 / 15.0 * p) - 1)))
    cq, cp = res[(32, "q105")]["classes"], res[(32, "plain")]["classes"]
    lines.append("Where the difference sits (bracketed ms per step, q105 / plain, against 52 / 15 = 3.47): "
                 + ", ".join("%s %.2f" % (k, cq[k]["ms"] / cp[k]["ms"]) for k in ("gemm", "dwconv", "bn", "head", "other") if cp[k]["ms"] > 0) + ".  " + EXPLAIN)
    if (32, "plain, parent revision") in med:
        a, b = med[(32, "plain")], med[(32, "plain, parent revision")]
        lines.append("")
        lines.append("The plain step on this tree against the parent revision (the depthwise tap-table records widened from 16 to 64 "
                     "layers, 1.8 KB of kernel arguments for the forward's first launch): %.3f ms against %.3f ms, %+.2f %%; the windows "
                     "of the two legs span %.3f-%.3f and %.3f-%.3f ms."
                     % (a, b, 100 * (a / b - 1), min(res[(32, "plain")]["ms"]), max(res[(32, "plain")]["ms"]),
                        min(res[(32, "plain, parent revision")]["ms"]), max(res[(32, "plain, parent revision")]["ms"])))
    lines += ["", "No test gates on time, and `bench.py` measures the plain variant only."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
