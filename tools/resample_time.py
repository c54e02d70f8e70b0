"""Dev tool: the two resampler launches profiles/resample_kernel.txt quotes, 10 of each after 3 warm-up launches, meant to run
under `rocprofv3 --kernel-trace --stats` (the kernel's own time) - it also prints event-timed microseconds per call:
  a. 32 rows, 441000 -> 160000 samples (10 s at 44.1 kHz -> 16 kHz), f32 -> f32
  b. 32 rows, 160000 samples at speed 0.9 (10/9: 177778 out), PCM16 -> PCM16
With `--summarise DIR OUT` it reads the rocpd database a rocprofv3 run left under DIR and writes OUT next to the bytes each
launch must move (input read once + output written once; the bank is 304 KB / under 1 KB and stays in L2).
python tools/resample_time.py            |   python tools/resample_time.py --summarise DIR profiles/resample_kernel.txt"""
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("a", "32 x 441000 -> 160000 samples (44100 -> 16000), f32 -> f32", "float, float", 32 * (441000 + 160000) * 4),
         ("b", "32 x 160000 -> 177778 samples (speed 0.9 = 10/9), PCM16 -> PCM16", "short, short", 32 * (160000 + 177778) * 2)]
STREAM_TBS = 6.29     # the streaming read these boxes achieve (README)


def run():
    import torch
    from lightning_asr_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    xa = (torch.rand(32, 441000, generator=g) * 1.8 - 0.9).to(dev)
    xb = torch.randint(-29000, 29000, (32, 160000), generator=g, dtype=torch.int64).to(torch.int16).to(dev)
    ra, rb = ops.Resampler([(44100, 16000)], dev), ops.Resampler([(9, 10)], dev)
    oa = torch.empty(32, 160000, device=dev)
    ob = torch.empty(32, 177778, dtype=torch.int16, device=dev)
    for name, fn in (("a", lambda: ra(xa, out=oa)), ("b", lambda: rb(xb, out=ob))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print("case %s: %.1f us per call (events around 10 launches)" % (name, e0.elapsed_time(e1) / 10 * 1e3))


def summarise(root, out_path):
    import sqlite3
    rows = []
    for p in glob.glob(os.path.join(root, "**", "*.db"), recursive=True):      # rocprofv3's rocpd database: the --stats view
        rows += list(sqlite3.connect(p).execute("select name, total_calls, total_duration, average from top_kernels"))
    lines = ["lasr_resample on one MI355X: `rocprofv3 --kernel-trace --stats -- python tools/resample_time.py` (13 launches per case, warm-up",
             "included in the average), kernel time next to the bytes the launch must move (input read once + output written once).",
             "For scale: a streaming read on these boxes reaches %.2f TB/s (README)." % STREAM_TBS, ""]
    for name, what, tmpl, nbytes in CASES:
        hit = [r for r in rows if "resample_kernel" in r[0] and tmpl in r[0]]
        if not hit:
            lines.append("case %s: %s: no resample_kernel<%s> row in the trace" % (name, what, tmpl))
            continue
        _, calls, _, avg_us = hit[0]
        lines.append("case %s: %s" % (name, what))
        lines.append("  calls %d, average %.1f us; %.1f MB to move -> %.2f TB/s effective; the same bytes at %.2f TB/s: %.1f us"
                     % (calls, avg_us, nbytes / 1e6, nbytes / avg_us / 1e6, STREAM_TBS, nbytes / STREAM_TBS / 1e6))
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], sys.argv[3])
    else:
        run()
