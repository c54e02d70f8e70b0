"""Dev tool: time lasr_ctc_align_long (W = 4096) per frame against lasr_ctc_align at the same 4095 states per step, in one
process, warm, device events, alternating rounds.  Planted inputs (tests/helpers/ctc_align_long_oracle.plant_path): labels uniform,
a random monotone alignment, logp = log_softmax(N(0,1) + 3 at the planted class), built on the device.
  long_hour   B=1 T'=180000 S=50000 C=28     an hour of English
  long_c4334  B=1 T'= 45000 S= 3000 C=4334   a quarter of an hour at AISHELL's vocabulary (780 MB of log-probs)
  full_2047   B=1 T'=  2001 S= 2047 C=28     lasr_ctc_align: four waves of 16 states per lane, the band's geometry without a band.
                                             2047 labels do not fit 2001 frames: the recursion runs in full, no backtrace follows
                                             (nothing planted: a random hot class per frame)
  full_1600   B=1 T'=  2001 S= 1600 C=28     the same four waves on a feasible, planted row: recursion + backtrace
  full_1600_c4334  the same at C=4334: what the emission gather from 17 KB rows costs the EXISTING kernel
Writes a markdown table (default profiles/ctc_align_long_time.md).
python tools/align_long_time.py [rounds] [out.md]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ctc_align_long_oracle as L  # noqa: E402
from lightning_asr_amd import _lib, ops  # noqa: E402

BAND = 4096
SHAPES = [("long_hour", True, 180000, 50000, 28, 3), ("long_c4334", True, 45000, 3000, 4334, 3), ("full_1600", False, 2001, 1600, 28, 40),
          ("full_1600_c4334", False, 2001, 1600, 4334, 40), ("full_2047", False, 2001, 2047, 28, 40)]


def planted_on_device(T, S, C, dev, seed):
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, C - 1, size=S).astype(np.int64)
    if S + L.n_repeats(labels.tolist()) <= T:
        path = torch.from_numpy(L.plant_path(labels.tolist(), T, C - 1, rng)).to(dev)
    else:
        path = torch.from_numpy(rng.randint(0, C, size=T).astype(np.int64)).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(T, C, generator=g, device=dev)
    x[torch.arange(T, device=dev), path] += 3.0
    return torch.log_softmax(x, -1).unsqueeze(0).contiguous(), torch.from_numpy(labels).to(dev).unsqueeze(0)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ctc_align_long_time.md")
    dev = torch.device("cuda")
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    cases = []
    for name, is_long, T, S, C, reps in SHAPES:
        logp, tg = planted_on_device(T, S, C, dev, 1)
        tl = torch.tensor([S], dtype=torch.int32, device=dev)
        if is_long:
            al = ops.ctc_align_long(logp, tg, None, tl, C - 1, band=BAND)
            nb = int(lib.lasr_ctc_align_long_workspace_bytes(1, T, S, BAND))
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)

            def fn(logp=logp, tg=tg, tl=tl, al=al, ws=ws, nb=nb, T=T, S=S, C=C):
                _lib.call("lasr_ctc_align_long", logp.data_ptr(), tg.data_ptr(), None, tl.data_ptr(), 1, T, C, S, C - 1, BAND,
                          al.score.data_ptr(), al.frame_state.data_ptr(), al.frame_logp.data_ptr(), al.label_start.data_ptr(),
                          al.label_end.data_ptr(), al.status.data_ptr(), al.band_lo.data_ptr(), ws.data_ptr(), nb, st)
            torch.cuda.synchronize()
            assert int(al.status[0]) == 0, "the planted path was lost"
            moves = int((al.band_lo[0, 1:] != al.band_lo[0, :-1]).sum())
        else:
            al = ops.ctc_align(logp, tg, None, tl, C - 1)
            nb = int(lib.lasr_ctc_align_workspace_bytes(1, T, S))
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)

            def fn(logp=logp, tg=tg, tl=tl, al=al, ws=ws, nb=nb, T=T, S=S, C=C):
                _lib.call("lasr_ctc_align", logp.data_ptr(), tg.data_ptr(), None, tl.data_ptr(), 1, T, C, S, C - 1, al.score.data_ptr(),
                          al.frame_state.data_ptr(), al.frame_logp.data_ptr(), al.label_start.data_ptr(), al.label_end.data_ptr(),
                          ws.data_ptr(), nb, st)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(al.score[0])) == (S + L.n_repeats(tg[0].tolist()) <= T)
            moves = 0
        cases.append({"name": name, "T": T, "S": S, "C": C, "reps": reps, "fn": fn, "ws": nb, "moves": moves, "us": []})
    for c in cases:                                        # warm: code objects loaded, caches in their steady state
        for _ in range(2):
            c["fn"]()
    torch.cuda.synchronize()
    for _ in range(rounds):                                # alternating rounds: every round times every case once
        for c in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(c["reps"]):
                c["fn"]()
            e1.record()
            torch.cuda.synchronize()
            c["us"].append(e0.elapsed_time(e1) / c["reps"] * 1e3)
    base = statistics.median(cases[-1]["us"]) / cases[-1]["T"]
    lines = ["# lasr_ctc_align_long at W = %d against lasr_ctc_align at 4095 states" % BAND, "",
             "`python tools/align_long_time.py %d`: one process, warm, device events around `reps` calls, %d alternating rounds; planted inputs."
             % (rounds, rounds), "",
             "| case | T' | S | C | band moves | workspace MB | reps | call ms (median) | call ms (min) | us per frame (median) | vs full_2047 |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in cases:
        med, mn = statistics.median(c["us"]), min(c["us"])
        lines.append("| %s | %d | %d | %d | %d | %.1f | %d | %.3f | %.3f | %.4f | %.2fx |"
                     % (c["name"], c["T"], c["S"], c["C"], c["moves"], c["ws"] / 1e6, c["reps"], med / 1e3, mn / 1e3, med / c["T"], med / c["T"] / base))
    lines += ["", "A call is the whole launch: the recursion, the backtrace and the span pass.  The full_* rows are the existing kernel",
              "on four waves of 16 states per lane (its backpointer table sits in the workspace at these shapes, as the banded kernel's",
              "always does); full_2047 is infeasible by count (2047 labels on 2001 frames), so its call is the recursion without a backtrace."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
