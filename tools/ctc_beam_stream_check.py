"""Did the Streamed mode of beam_search_kernel change what the one-shot searches compile to?  Compiles the device side of
lightning_asr_amd/csrc/ctc_beam.hip for gfx950 at a parent revision and in the tree (no GPU needed), with the flags the Makefile
gives that file, and writes profiles/ctc_beam_stream_check.txt: per one-shot instantiation VGPRs, static LDS, scratch and a hash
of the instruction stream on both sides, then the Streamed instantiations' own figures.

    python tools/ctc_beam_stream_check.py [--parent HEAD^] [--out profiles/ctc_beam_stream_check.txt]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import beam_kernel_resources as bkr  # noqa: E402

SRC = os.path.join("lightning_asr_amd", "csrc", "ctc_beam.hip")
FLAGS = ["-mllvm", "-pragma-unroll-threshold=32768"]        # Makefile: build/ctc_beam.o


def compile_kernels(src):
    asm = os.path.join(tempfile.mkdtemp(), "ctc_beam.s")
    subprocess.run(["hipcc"] + bkr.BASE + FLAGS + ["-o", asm, src], check=True, stderr=subprocess.DEVNULL)
    out = {}
    for name, r in bkr.kernels(asm).items():
        out[(bkr.short(name), "Streamed" in name)] = r
    return out


def row(r):
    return "vgprs %3d  lds %5d  scratch %4d  code %s" % (r["vgpr_count"], r["group_segment_fixed_size"],
                                                        r["private_segment_fixed_size"], r["code"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD^")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_beam_stream_check.txt"))
    a = ap.parse_args()
    # the parent's file goes next to the tree's, so that its includes resolve
    old_src = os.path.join(ROOT, os.path.dirname(SRC), "_parent_ctc_beam_check.hip")
    try:
        with open(old_src, "wb") as f:
            f.write(subprocess.run(["git", "show", "%s:%s" % (a.parent, SRC)], cwd=ROOT, check=True, stdout=subprocess.PIPE).stdout)
        old = compile_kernels(old_src)
    finally:
        if os.path.exists(old_src):
            os.remove(old_src)
    new = compile_kernels(os.path.join(ROOT, SRC))
    rev = subprocess.run(["git", "rev-parse", "--short", a.parent], cwd=ROOT, check=True, stdout=subprocess.PIPE).stdout.decode().strip()
    lines = ["ctc_beam.hip on gfx950, hipcc -O3 %s: the parent (%s) against this tree." % (" ".join(FLAGS), rev),
             "vgprs: VGPRs and AGPRs together; lds / scratch in bytes; code: md5 of the instruction stream, block labels renumbered.",
             "", "One-shot instantiations (Mode = OneShot), parent -> tree:"]
    differ = 0
    key = lambda kv: (kv[0][0].split("<")[0], len(kv[0][0]), kv[0][0])
    for (name, streamed), r in sorted(old.items(), key=key):
        n = new.get((name, False))
        if n is None:
            lines.append("  %-46s MISSING in the tree" % name)
            differ += 1
            continue
        same_res = all(r[k] == n[k] for k in ("vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size"))
        same = same_res and r["code"] == n["code"]
        differ += not same
        lines.append("  %-46s %s" % (name, row(r)))
        lines.append("  %-46s %s  %s" % ("", row(n), "identical" if same else "SAME RESOURCES, other code" if same_res else "DIFFERENT"))
    lines += ["", "%d of %d one-shot kernels differ from the parent." % (differ, len(old)), "",
              "Streamed instantiations (lasr_ctc_beam_stream_feed), tree only:"]
    for (name, streamed), r in sorted(new.items(), key=key):
        if streamed:
            lines.append("  %-46s %s" % (name, row(r)))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
