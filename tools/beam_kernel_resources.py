"""Per-kernel resources of lightning_asr_amd/csrc/ctc_beam.hip on gfx950, and whether a change of source or of compiler flags
alters a kernel's instructions.  Compiles the device side of each given source to assembly (no GPU needed), once per flag set,
and prints one JSON line per kernel: VGPRs (VGPRs and AGPRs together), SGPRs, static LDS, scratch, and a hash of its instruction
stream (comments and directives removed, block labels renumbered), so that two builds of a kernel compare by that hash.

    python tools/beam_kernel_resources.py [--src FILE.hip ...] [--flags "" "-mllvm -pragma-unroll-threshold=32768"] [--out F.jsonl]

--src defaults to the tree's ctc_beam.hip; another revision of the file (git show REV:lightning_asr_amd/csrc/ctc_beam.hip > f.hip,
placed next to the tree's so that its includes resolve) can be given beside it."""
import argparse
import hashlib
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include")]
META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")


def short(name):
    """beam_search_kernel<LmScorer<true>, J=33> from the mangled name (beam_search_lm_kernel<33, true> for a revision of the
    file with one kernel per scorer)"""
    m = re.search(r"\d+beam_search_kernelILi(\d+)E\w*?\d+([A-Za-z]+Scorer)(?:ILb([01])E)?", name)
    if m:
        scorer = m.group(2) + {"0": "<false>", "1": "<true>", None: ""}[m.group(3)]
        return "beam_search_kernel<%s, J=%s>" % (scorer, m.group(1))
    m = re.search(r"\d+(beam_\w+?_kernel)(?:IL[ij](\d+)E(?:Lb([01])E)?E)?", name)
    if not m:
        return name
    args = [a for a in (m.group(2), {"0": "false", "1": "true", None: None}[m.group(3)]) if a is not None]
    return m.group(1) + ("<%s>" % ", ".join(args) if args else "")


def kernels(asm_path):
    body, cur, items = {}, None, []
    for line in open(asm_path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            elif not line.lstrip().startswith(";"):
                text = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())
                if text and (not text.startswith(".") or text.startswith(".LBB")):      # instructions and labels, no directives
                    body[cur].append(text)
            continue
        # the metadata: one YAML list item per kernel, its keys in alphabetical order (.name in the middle)
        if re.match(r"^  - \.", line):
            items.append({})
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)", line)
        if m and items and (m.group(1) in META or m.group(1) == "name"):
            items[-1][m.group(1)] = m.group(2)
    out = {}
    for it in items:
        if "name" in it and it["name"] in body:
            out[it["name"]] = dict({k: int(it[k]) for k in META if k in it},
                                   code=hashlib.md5("\n".join(body[it["name"]]).encode()).hexdigest()[:12])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", nargs="+", default=[os.path.join(ROOT, "lightning_asr_amd", "csrc", "ctc_beam.hip")])
    ap.add_argument("--flags", nargs="+", default=["", "-mllvm -pragma-unroll-threshold=32768"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    lines = []
    for src in a.src:
        for i, flags in enumerate(a.flags):
            asm = os.path.join(tmp, "%s.%d.s" % (os.path.basename(src), i))
            subprocess.run(["hipcc"] + BASE + shlex.split(flags) + ["-o", asm, src], check=True, stderr=subprocess.DEVNULL)
            for name, r in sorted(kernels(asm).items(), key=lambda kv: (re.sub(r'<.*', '', short(kv[0])), len(short(kv[0])), short(kv[0]))):
                lines.append({"src": os.path.relpath(src, ROOT), "flags": flags, "kernel": short(name), "vgprs": r.get("vgpr_count"),
                              "sgprs": r.get("sgpr_count"), "lds_bytes": r.get("group_segment_fixed_size"),
                              "scratch_bytes": r.get("private_segment_fixed_size"), "spilled_vgprs": r.get("vgpr_spill_count"),
                              "code_md5": r["code"]})
    out = open(a.out, "w") if a.out else sys.stdout
    for r in lines:
        out.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
