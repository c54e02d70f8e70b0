"""Cases, operands and the f64 CPU reference of the depthwise-convolution parity tests (tests/test_gpu_dwconv.py, its worker
tests/helpers/dwconv_probe.py and the host checks in tests/test_host_dwconv_cases.py).

Operands.  Three kinds, all seeded:
  * "int": small integers - x and dy are non-zero with probability 0.25 (values +-1, +-2), every tap of w is +-1 or +-2, the addend
    is an integer in [-8, 8].  Every product and every partial sum is then an integer far below 256 (exact in bf16) resp. 2^24
    (exact in f32), whatever the order of summation: the kernels must match the reference BIT FOR BIT, and a tap that is misplaced,
    dropped or counted twice is a wrong integer.  `exactness` states the condition; every comparison asserts it on its own reference.
  * "pos": x (and dy) one-hot at frames no closer than k apart - frame 0, T - 1 and both sides of every tile edge the kernels have,
    dealt over the channels - and w[c][j] = 1 + (j + 3 c) % 200: every output element is the value of the one tap that landed on it.
  * "rand": randn operands rounded to the tensor's dtype (taps to bf16 for bf16 tensors, as the kernels round them), for the
    tolerance pass.

Reference (f64, CPU): forward F.conv1d; data gradient the same with the taps reversed, plus the addend; weight gradient the explicit
correlation sum_{b,t} dy[b,t,c] * xpad[b, t*stride + j, c].  Tensors are channels-last (B, T, C) as the library takes them.
"""
from __future__ import annotations

import math
import sys
from collections import namedtuple

import torch
import torch.nn.functional as F

Case = namedtuple("Case", "name dtype B T C k stride kind group")

# both sides of every time-tile edge of the stride-1 kernels: 128 (VALU forward), 256 (half tiles, unified backward, VALU weight
# gradient chunks), 288 (MFMA weight gradient), 512 (full tiles), and their multiples inside T = 700
TILE_EDGES = (127, 128, 255, 256, 287, 288, 383, 384, 511, 512, 575, 576, 639, 640)


def conv_out_len(Tin: int, k: int, stride: int) -> int:
    return (Tin + 2 * (k // 2) - k) // stride + 1


def _c(dtype, B, T, C, k, stride=1, kind="int", group=""):
    name = "%s_s%d_B%d_T%d_C%d_k%d" % (dtype, stride, B, T, C, k) + ("_pos" if kind == "pos" else "")
    return Case(name, dtype, B, T, C, k, stride, kind, group)


def _table():
    t = []
    # ---- bf16, stride 1
    for k in (1, 3, 17, 19, 49, 51, 81, 83, 101, 103, 111, 113, 115, 127):
        t.append(_c("bf16", 2, 300, 72, k, group="k sweep"))
    for k in (33, 87):
        for T in (1, 7, 15, 16, 17, 255, 256):
            t.append(_c("bf16", 2, T, 64, k, group="short and single-tile"))
    for T in (257, 511, 512, 513):
        t.append(_c("bf16", 2, T, 64, 33, group="half-tile edges"))
    for T in (272, 273, 560, 561):
        t.append(_c("bf16", 2, T, 64, 33, group="weight-gradient tile edges"))
    t.append(_c("bf16", 1, 2049, 64, 87, group="tile loops"))
    t.append(_c("bf16", 3, 1300, 72, 33, group="tile loops"))
    t.append(_c("bf16", 3, 1300, 72, 87, group="tile loops"))
    for k in (33, 87):
        t.append(_c("bf16", 100, 600, 64, k, group="full tiles"))
    for C in (8, 40, 200, 336):
        t.append(_c("bf16", 2, 300, C, 51, group="channel remainders"))
    for k in (5, 75, 113):
        t.append(_c("bf16", 1, 700, 72, k, kind="pos", group="position-coded"))
    # full-tile instances of the narrow and the 3-step windows (T <= 256 never takes half tiles), and the narrow windows that the
    # unified backward hands to the two-kind grid, over a tile loop
    for k in (3, 17, 51, 75):
        t.append(_c("bf16", 2, 200, 72, k, group="full tiles, one per utterance"))
    for k in (5, 17):
        t.append(_c("bf16", 3, 1300, 72, k, group="narrow windows over a tile loop"))
    # ---- f32, stride 1: a cross-section of C x T x k
    for (C, T, k) in ((4, 1, 1), (4, 127, 39), (4, 128, 41), (4, 129, 63), (4, 257, 65), (4, 257, 127),
                      (68, 1, 127), (68, 127, 65), (68, 128, 63), (68, 129, 41), (68, 257, 39), (68, 257, 1),
                      (68, 129, 127), (4, 128, 1)):
        t.append(_c("f32", 2, T, C, k, group="f32"))
    # ---- stride 2, both dtypes
    s2 = [(Tin, k, C) for Tin in (1, 2, 127, 128, 129, 255, 256, 257) for k in (1, 33, 127) for C in (4, 64, 72)]
    # a cross-section of the product: every Tin with every k, the channel counts dealt round
    for i, (Tin, k, C) in enumerate(s2):
        if (i // 3 + i) % 3 == 0:
            for dt in ("f32", "bf16"):
                t.append(_c(dt, 2, Tin, C, k, stride=2, group="stride 2"))
    for dt in ("f32", "bf16"):
        t.append(_c(dt, 100, 255, 128, 33, stride=2, group="stride 2, R = 8"))
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return t


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}


def torch_dtype(case):
    return torch.bfloat16 if case.dtype == "bf16" else torch.float32


def _seed(case):
    return (case.B * 1000003 + case.T * 10007 + case.C * 101 + case.k * 7 + case.stride) % (2 ** 31)


def _sparse_ints(shape, g):
    nz = torch.rand(shape, generator=g) < 0.25
    mag = torch.randint(1, 3, shape, generator=g).double()
    sgn = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return nz.double() * mag * sgn


def impulse_frames(T: int, k: int, c: int):
    """frames of channel c's impulses: a greedy walk over 0, T - 1 and the tile edges, started at a different candidate per channel,
    keeping a frame when it is at least k away from every frame kept so far"""
    cand = [0, T - 1] + [e for e in TILE_EDGES if 0 < e < T - 1]
    rot = c % len(cand)
    keep = []
    for f in cand[rot:] + cand[:rot]:
        if all(abs(f - g) >= k for g in keep):
            keep.append(f)
    return sorted(keep)


def operands(case, kind=None):
    """x (B, Tin, C), w (C, k), dy (B, Tout, C), addend (B, Tout, C) as f64 CPU tensors holding values the case's dtype represents"""
    kind = kind or case.kind
    B, T, C, k = case.B, case.T, case.C, case.k
    Tout = conv_out_len(T, k, case.stride)
    g = torch.Generator().manual_seed(_seed(case) + (1 if kind == "rand" else 0))
    if kind == "int":
        x = _sparse_ints((B, T, C), g)
        dy = _sparse_ints((B, Tout, C), g)
        w = (torch.randint(1, 3, (C, k), generator=g).double()) * (torch.randint(0, 2, (C, k), generator=g).double() * 2 - 1)
        add = torch.randint(-8, 9, (B, Tout, C), generator=g).double()
    elif kind == "pos":
        assert case.stride == 1
        x = torch.zeros(B, T, C, dtype=torch.float64)
        for c in range(C):
            x[:, impulse_frames(T, k, c), c] = 1.0
        dy = x.roll(1, dims=2).clone()                        # the same impulses, dealt to the next channel
        j = torch.arange(k).view(1, k)
        cc = torch.arange(C).view(C, 1)
        w = (1 + (j + 3 * cc) % 200).double()
        add = torch.randint(-8, 9, (B, Tout, C), generator=g).double()
    elif kind == "rand":
        dt = torch_dtype(case)
        x = torch.randn(B, T, C, generator=g).to(dt).double()
        dy = torch.randn(B, Tout, C, generator=g).to(dt).double()
        w = (torch.randn(C, k, generator=g) / math.sqrt(k)).to(dt).double()
        add = torch.randn(B, Tout, C, generator=g).to(dt).double()
    else:
        raise ValueError(kind)
    return x, w, dy, add


def ref_fwd(x, w, stride=1):
    """(B, Tin, C) f64, (C, k) f64 -> (B, Tout, C) f64"""
    C, k = w.shape
    y = F.conv1d(x.transpose(1, 2), w.view(C, 1, k), None, stride, k // 2, 1, C)
    return y.transpose(1, 2).contiguous()


def ref_dgrad(dy, w, addend=None):
    dx = ref_fwd(dy, w.flip(1), 1)
    return dx if addend is None else dx + addend


def ref_wgrad(x, dy, k, stride=1):
    """dW[c][j] = sum_{b,t} dy[b,t,c] * xpad[b, t*stride + j, c]"""
    pad = k // 2
    Tout = dy.shape[1]
    xp = F.pad(x, (0, 0, pad, pad))
    return torch.stack([(dy * xp[:, j:j + (Tout - 1) * stride + 1:stride, :]).sum(dim=(0, 1)) for j in range(k)], dim=1)


def reference(case, kind=None):
    """{op: f64 reference} for the case's ops, from operands(case, kind)"""
    x, w, dy, add = operands(case, kind)
    out = {"fwd": ref_fwd(x, w, case.stride), "wgrad": ref_wgrad(x, dy, case.k, case.stride)}
    if case.stride == 1:
        out["dgrad"] = ref_dgrad(dy, w, add)
        out["bwd"] = ref_dgrad(dy, w, None)
        out["bwd_add"] = out["dgrad"]
    return out


def exactness(ref):
    """the condition under which integer operands make every kernel form exact: outputs representable in bf16 (|v| <= 256), weight
    gradients in f32 (|v| < 2^24), everything an integer.  Returns (ok, worst |y| / |dx|, worst |dW|)."""
    ymax = max(float(ref[o].abs().max()) for o in ref if o != "wgrad")
    wmax = float(ref["wgrad"].abs().max())
    ints = all(bool((ref[o] == ref[o].round()).all()) for o in ref)
    return ints and ymax <= 256 and wmax < 2 ** 24, ymax, wmax


# ------------------------------------------------------------------------------------------- the GPU side (shared with the worker)
def run_ops(case, dev, kind=None):
    """every op of the case on the GPU: {op: CPU tensor}, "wgrad" f32 (C, k), "bwd*" -> (dx, dW) split into op and op + "_dw" """
    from lightning_asr_amd import ops
    x, w, dy, add = operands(case, kind)
    dt = torch_dtype(case)
    xg, dyg, addg = x.to(dt).to(dev), dy.to(dt).to(dev), add.to(dt).to(dev)
    wg = w.float().to(dev)
    out = {"fwd": ops.dwconv(xg, wg, case.stride).cpu(), "wgrad": ops.dwconv_wgrad(xg, dyg, case.k, case.stride).cpu()}
    if case.stride == 1:
        out["dgrad"] = ops.dwconv(dyg, wg, 1, flip=True, addend=addg).cpu()
        dw, dx = ops.dwconv_bwd_fused(xg, dyg, wg, None)
        out["bwd"], out["bwd_dw"] = dx.cpu(), dw.cpu()
        dw, dx = ops.dwconv_bwd_fused(xg, dyg, wg, addg)
        out["bwd_add"], out["bwd_add_dw"] = dx.cpu(), dw.cpu()
    return out


def ref_of(ref, op):
    return ref["wgrad"] if op.endswith("_dw") else ref[op]


def plan_of(case):
    from lightning_asr_amd import _lib
    return _lib.dwconv_plan(case.B, case.T, case.C, case.k, case.stride, _lib.BF16 if case.dtype == "bf16" else _lib.F32)


def form_of(plan, op):
    """the kernel form that computes `op` under `plan` (labels of failures and of the measured record)"""
    if op == "fwd" or op == "dgrad":
        return "fwd:%s/nks%d/nset%d" % (plan["fwd_form"], plan["nks"], plan["nset"]) if plan["fwd_form"] == "mfma" else \
            "fwd:%s%s" % (plan["fwd_form"], "/r%d" % plan["fwd_r"] if plan["fwd_r"] else "")
    if op == "wgrad":
        return "wgrad:%s" % plan["wgrad_form"] + ("/z%d" % plan["zsplit"] if plan["wgrad_form"] == "mfma" else
                                                  "/ts%d" % plan["ts"] if plan["wgrad_form"] == "valu" else "")
    return "bwd:%s" % plan["bwd_form"] + ("/nks%d" % plan["nks"] if plan["bwd_form"] != "two_launches" else "")


def exact_mismatches(case, got, ref):
    """bit-for-bit comparison of every op's result with the reference in the op's storage type: a list of
    {op, wrong, first, got, want} (first = (b, t, c) or (c, j) of the first wrong element)"""
    bad = []
    for op, g in got.items():
        want = ref_of(ref, op).to(g.dtype)
        if g.shape != want.shape:
            bad.append({"op": op, "wrong": -1, "first": list(g.shape), "got": 0.0, "want": 0.0})
            continue
        ne = (g != want) | torch.isnan(g)
        n = int(ne.sum())
        if n:
            idx = tuple(int(i) for i in ne.nonzero()[0])
            bad.append({"op": op, "wrong": n, "first": list(idx), "got": float(g[idx]), "want": float(want[idx])})
    return bad


# tolerances of the random pass: the ones the project's depthwise tests already hold these ops to (tests/test_gpu_ops.py)
def rand_errors(case, got, ref):
    """{op: (error, gate)}, both relative to max |ref|: forward / data gradient max |err| against 4e-3 (bf16: one rounding of the
    result) or 2e-6 (f32); weight gradient max |err| against 2e-5 * max |ref| + 1e-6 (bf16) or 2e-5 * max |ref| (f32)"""
    out = {}
    for op, g in got.items():
        want = ref_of(ref, op)
        err = float((g.double() - want).abs().max())
        scale = float(want.abs().max())
        if torch.isnan(g).any():
            err = float("inf")
        if op == "wgrad" or op.endswith("_dw"):      # err < 2e-5 * scale + 1e-6, written relative to the scale
            out[op] = (err / (scale + 1e-30), 2e-5 + (1e-6 / (scale + 1e-30) if case.dtype == "bf16" else 0.0))
        else:
            out[op] = (err / (scale + 1e-30), 4e-3 if case.dtype == "bf16" else 2e-6)
    return out


def plan_key(plan):
    """the part of a plan that selects code: forms, template instances, and whether the grids split the time axis"""
    return (plan["fwd_form"], plan["nks"], plan["nset"], plan["gz_d"] > 1, plan["fwd_r"], plan["wgrad_form"], plan["zsplit"], plan["ts"],
            plan["bwd_form"], plan["bwd_gz"] > 1, plan["bwd_wgs_launched"] > plan["bwd_wgs"], plan["bwd_tiles"] > plan["bwd_gz"])


def one_case_per_plan(cases):
    """the smallest case of every distinct plan_key (per dtype and stride)"""
    seen = {}
    for c in sorted(cases, key=lambda c: (c.B * c.T * c.C, c.name)):
        seen.setdefault((c.dtype, c.stride, plan_key(plan_of(c))), c)
    return list(seen.values())


def worker_cases():
    """what the switch children run: the bf16 stride-1 part of the table and the stride-2 cases"""
    return [c for c in TABLE if c.stride == 2 or c.dtype == "bf16"]


def coverage_gaps(plans):
    """what the table has to reach under default switches, checked on {case name: plan}: a list of the items it does not reach"""
    P = list(plans.values())
    gaps = []
    inst = {(p["nks"], p["nset"]) for p in P if p["fwd_form"] == "mfma"}
    for want in [(n, s) for n in (1, 2, 3, 4) for s in (1, 2)]:
        if want not in inst:
            gaps.append("forward instance nks=%d nset=%d" % want)
    for z in (1, 2):
        if not any(p["wgrad_form"] == "mfma" and p["zsplit"] == z for p in P):
            gaps.append("MFMA weight gradient with zsplit %d" % z)
    checks = {
        "VALU weight gradient on bf16 (k > 111)": lambda n, p: n.startswith("bf16_s1") and p["wgrad_form"] == "valu",
        "VALU forward on bf16 (k > 113)": lambda n, p: p["fwd_form"] == "valu",
        "MFMA forward with the VALU weight gradient (k = 113)": lambda n, p: p["fwd_form"] == "mfma" and p["wgrad_form"] == "valu",
        "unified 32-channel backward with gz > 1": lambda n, p: p["bwd_form"] == "uni32" and p["bwd_gz"] > 1,
        "unified 64-channel backward with gz > 1": lambda n, p: p["bwd_form"] == "uni64" and p["bwd_gz"] > 1,
        "unified 32-channel backward, idle workgroups in the grid": lambda n, p: p["bwd_form"] == "uni32" and p["bwd_wgs_launched"] > p["bwd_wgs"],
        "unified 64-channel backward, idle workgroups in the grid": lambda n, p: p["bwd_form"] == "uni64" and p["bwd_wgs_launched"] > p["bwd_wgs"],
        "unified 32-channel backward, more tiles than gz": lambda n, p: p["bwd_form"] == "uni32" and p["bwd_tiles"] > p["bwd_gz"] > 1,
        "unified 64-channel backward, more tiles than gz": lambda n, p: p["bwd_form"] == "uni64" and p["bwd_tiles"] > p["bwd_gz"] > 1,
        "two-kind backward grid for the narrow windows": lambda n, p: p["bwd_form"] == "two_kind",
        "forward half tiles over gz_d = 8": lambda n, p: p["nset"] == 1 and p["gz_d"] == 8,
        "forward full tiles, several per utterance": lambda n, p: p["nset"] == 2 and BY_NAME[n].T > 512,
        "strided forward R = 4": lambda n, p: p["fwd_r"] == 4,
        "strided forward R = 8": lambda n, p: p["fwd_r"] == 8,
        "f32 forward": lambda n, p: p["fwd_form"] == "f32",
    }
    for ts in (1, 2, 3):
        checks["f32 weight gradient ts = %d" % ts] = lambda n, p, ts=ts: n.startswith("f32_s1") and p["ts"] == ts
    for what, f in checks.items():
        if not any(f(n, p) for n, p in plans.items()):
            gaps.append(what)
    return gaps


def switch_gaps(env, plans):
    """under the switch set `env` the named alternative form is the one chosen: a list of the cases where it is not.  `plans` are
    the child's own plans of worker_cases()."""
    s1 = {n: p for n, p in plans.items() if BY_NAME[n].stride == 1}
    bad = []

    def need(cond, n, p):
        if not cond:
            bad.append((n, p))

    key = sorted(env.items())
    if key == [("LASR_DWCONV_FMA", "1")]:
        for n, p in s1.items():
            need(p["fwd_form"] == "fma" and p["bwd_form"] == "two_launches", n, p)
    elif key == [("LASR_DWCONV_DOT2", "1")]:
        for n, p in s1.items():
            need(p["fwd_form"] == "valu" and p["bwd_form"] == "two_launches", n, p)
    elif key == [("LASR_DWWGRAD_VALU", "1")]:
        for n, p in s1.items():
            need(p["wgrad_form"] == "valu" and p["bwd_form"] == "two_launches", n, p)
    elif key == [("LASR_DW_UNI", "0")]:
        for n, p in s1.items():
            need(p["bwd_form"] == ("two_kind" if p["fwd_form"] == "mfma" and p["wgrad_form"] == "mfma" else "two_launches"), n, p)
    elif key == [("LASR_DW_UNI", "64")]:
        for n, p in s1.items():
            need(p["bwd_form"] != "uni32", n, p)
        need(sum(p["bwd_form"] == "uni64" and p["nks"] <= 3 for p in s1.values()) >= 10, "uni64 at nks <= 3", {})
    elif key == [("LASR_DW_NO_FUSED_BWD", "1")]:
        for n, p in s1.items():
            need(p["bwd_form"] == "two_launches", n, p)
    elif key == [("LASR_DWCONV_NO_HALF", "1")]:
        for n, p in s1.items():
            need(p["fwd_form"] != "mfma" or (p["nset"] == 2 and p["gz_d"] == 1), n, p)
        need(any(p["nset"] == 2 and BY_NAME[n].T > 512 and BY_NAME[n].B < 100 for n, p in s1.items()), "full tiles in a loop", {})
    elif key == [("LASR_DWWGRAD_ZSPLIT", "8")]:
        need(max(p["zsplit"] for p in s1.values()) == 8, "zsplit 8", {})
        need(any(p["zsplit"] == 4 for p in s1.values()), "zsplit 4", {})
    else:
        raise ValueError(env)
    return bad


RAND = "#rand"      # key suffix of a case's random-pass reference


def save_refs(path, refs):
    """references as compact tensors: integer outputs as int16 and integer weight gradients as f32 (both exact under `exactness`),
    the random pass's in f64"""
    torch.save({n: r if n.endswith(RAND) else {op: (t.float() if op == "wgrad" else t.to(torch.int16)) for op, t in r.items()}
                for n, r in refs.items()}, path)


def load_refs(path):
    return {n: {op: t.double() for op, t in r.items()} for n, r in torch.load(path).items()}


def exact_pass(case, dev, ref):
    """the case's ops on its own operands against `ref`, bit for bit: mismatches labelled with the case and the form that ran"""
    plan = plan_of(case)
    bad = exact_mismatches(case, run_ops(case, dev), ref)
    for m in bad:
        m.update(case=case.name, form=form_of(plan, m["op"]))
    return bad


def rand_pass(cases, dev, ref_of_case):
    """randn operands, one case per distinct plan, at the project's tolerances: ({form: worst relative error}, [failures]);
    ref_of_case(case) -> the case's "rand" reference"""
    figures, fails = {}, []
    for c in one_case_per_plan(cases):
        plan = plan_of(c)
        for op, (err, gate) in rand_errors(c, run_ops(c, dev, "rand"), ref_of_case(c)).items():
            form = "%s %s %s" % (c.dtype, form_of(plan, op), "dW" if op == "wgrad" or op.endswith("_dw") else "out")
            print("%-30s %-10s %-36s %.3e (gate %.3e)" % (c.name, op, form, err, gate), file=sys.stderr)
            figures[form] = max(figures.get(form, 0.0), err)
            if not err <= gate:
                fails.append({"case": c.name, "op": op, "form": form, "err": err, "gate": gate})
    return figures, fails


def run_table(cases, dev, refs=None):
    """The whole check of `cases` in this process (the worker's job).  Returns {"plans": {name: plan}, "not_exact": [names],
    "mismatches": [...], "rand": {form: worst relative error}, "rand_fail": [...]}"""
    refs = refs if refs is not None else {}
    res = {"plans": {c.name: plan_of(c) for c in cases}, "mismatches": [], "not_exact": []}
    for c in cases:
        ref = refs.get(c.name) or reference(c)
        if not exactness(ref)[0]:
            res["not_exact"].append(c.name)
            continue
        res["mismatches"] += exact_pass(c, dev, ref)
    res["rand"], res["rand_fail"] = rand_pass(cases, dev, lambda c: refs.get(c.name + RAND) or reference(c, "rand"))
    return res
