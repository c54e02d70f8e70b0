"""CPU tier of the depthwise parity tests: the f64 reference of tests/helpers/dwconv_cases.py against a naive triple loop, the
exactness condition of the integer operands over the whole case table, the position-coded impulses, the output lengths, and - through
lasr_dwconv_plan, which launches nothing - the table's coverage of the kernel forms under default switches."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import dwconv_cases as D  # noqa: E402


def _naive(x, w, dy, add, stride):
    """y, dx (+ add), dW by the definition, one scalar at a time"""
    B, T, C = x.shape
    k = w.shape[1]
    pad = k // 2
    Tout = (T + 2 * pad - k) // stride + 1
    y = torch.zeros(B, Tout, C, dtype=torch.float64)
    dw = torch.zeros(C, k, dtype=torch.float64)
    dx = add.clone() if stride == 1 else None
    for b in range(B):
        for t in range(Tout):
            for j in range(k):
                ti = t * stride + j - pad
                if 0 <= ti < T:
                    y[b, t] += w[:, j] * x[b, ti]
                    dw[:, j] += dy[b, t] * x[b, ti]
                    if stride == 1:
                        dx[b, ti] += w[:, j] * dy[b, t]      # the forward's adjoint: what the flipped-tap correlation computes
    return y, dx, dw


def test_reference_equals_the_naive_loop():
    for dtype, T, C, k, stride in [("f32", 9, 4, 5, 1), ("f32", 1, 4, 3, 1), ("bf16", 12, 8, 7, 1), ("f32", 10, 4, 5, 2), ("f32", 11, 4, 5, 2),
                                   ("bf16", 1, 4, 3, 2), ("f32", 2, 4, 1, 2), ("f32", 6, 4, 9, 1)]:
        case = D.Case("tiny", dtype, 2, T, C, k, stride, "int", "")
        for kind in ("int", "rand"):
            x, w, dy, add = D.operands(case, kind)
            ref = D.reference(case, kind)
            y, dx, dw = _naive(x, w, dy, add, stride)
            assert ref["fwd"].shape == (2, D.conv_out_len(T, k, stride), C)
            tol = 0.0 if kind == "int" else 1e-12
            assert (ref["fwd"] - y).abs().max() <= tol, (case, kind)
            assert (ref["wgrad"] - dw).abs().max() <= tol, (case, kind)
            if stride == 1:
                assert (ref["dgrad"] - dx).abs().max() <= tol, (case, kind)
                assert (ref["bwd"] - (dx - add)).abs().max() <= tol and ref["bwd_add"] is ref["dgrad"]


def test_every_case_meets_the_exactness_condition():
    worst_y = worst_w = 0.0
    for case in D.TABLE:
        x, w, dy, add = D.operands(case)
        dt = D.torch_dtype(case)
        for t in (x, w, dy, add):
            assert torch.equal(t.to(dt).double(), t), case.name          # the operands themselves are exact in the case's dtype
        assert bool((w != 0).all()), case.name                           # every tap counts: a dropped one shows
        ok, ymax, wmax = D.exactness(D.reference(case))
        assert ok, (case.name, ymax, wmax)
        worst_y, worst_w = max(worst_y, ymax), max(worst_w, wmax)
    print("worst |y|, |dx| = %g, worst |dW| = %g over %d cases" % (worst_y, worst_w, len(D.TABLE)))


def test_position_coded_impulses_never_overlap_and_reach_every_edge():
    pos = [c for c in D.TABLE if c.kind == "pos"]
    assert sorted(c.k for c in pos) == [5, 75, 113]
    for case in pos:
        seen = set()
        for c in range(case.C):
            fr = D.impulse_frames(case.T, case.k, c)
            assert all(b - a >= case.k for a, b in zip(fr, fr[1:])) and 0 <= fr[0] and fr[-1] < case.T, (case.name, c, fr)
            seen.update(fr)
        want = {0, case.T - 1} | {e for e in D.TILE_EDGES if e < case.T - 1}
        assert want <= seen, (case.name, sorted(want - seen))
        x, w, dy, add = D.operands(case)
        assert int(w.max()) <= 200 and int(w.min()) >= 1
        y = D.reference(case)["fwd"]
        # every output element is one tap of its channel or nothing: the impulse at frame f puts w[c][j] at frame f + pad - j
        for c in (0, 1, case.C - 1):
            for f in D.impulse_frames(case.T, case.k, c):
                for j in (0, case.k // 2, case.k - 1):
                    t = f + case.k // 2 - j
                    if 0 <= t < case.T:
                        assert y[0, t, c] == w[c, j], (case.name, c, f, j)
        assert int((y != 0).sum()) <= int(x.sum()) * case.k


def test_output_lengths_match_conv_out_len():
    import torch.nn.functional as F
    for case in D.TABLE:
        Tout = D.conv_out_len(case.T, case.k, case.stride)
        assert Tout == (case.T if case.stride == 1 else (case.T - 1) // 2 + 1), case.name
        x, w, dy, add = D.operands(case)
        assert dy.shape == add.shape == (case.B, Tout, case.C) and x.shape == (case.B, case.T, case.C) and w.shape == (case.C, case.k)
        # the rule of include/lasr.h, Tout = (Tin + 2*(k/2) - k)/stride + 1, is nn.Conv1d's with padding k/2
        assert F.conv1d(torch.zeros(1, 1, case.T), torch.zeros(1, 1, case.k), None, case.stride, case.k // 2).shape[2] == Tout


def test_table_reaches_every_form_under_default_switches():
    """the dispatch facts the table is built on, confirmed by the library's own dispatch code (lasr_dwconv_plan launches nothing)"""
    plans = {c.name: D.plan_of(c) for c in D.TABLE}
    assert D.coverage_gaps(plans) == []
    P = lambda B, T, C, k: D.plan_of(D.Case("q", "bf16", B, T, C, k, 1, "int", ""))
    # the hand-overs by k: MFMA forward to 113, MFMA weight gradient to 111, the unified backward from 19 to 111
    assert [P(2, 300, 72, k)["fwd_form"] for k in (101, 113, 115, 127)] == ["mfma", "mfma", "valu", "valu"]
    assert [P(2, 300, 72, k)["wgrad_form"] for k in (101, 111, 113)] == ["mfma", "mfma", "valu"]
    assert [P(2, 300, 72, k)["bwd_form"] for k in (1, 17, 19, 75, 81, 83, 111, 113)] == \
        ["two_kind", "two_kind", "uni32", "uni32", "uni32", "uni64", "uni64", "two_launches"]
    assert [P(2, 300, 72, k)["nks"] for k in (17, 19, 49, 51, 81, 83)] == [1, 2, 2, 3, 3, 4]
    # the tile loops the issue names
    assert {k: P(1, 2049, 64, 87)[k] for k in ("nset", "gz_d", "bwd_gz", "bwd_tiles")} == {"nset": 1, "gz_d": 8, "bwd_gz": 8, "bwd_tiles": 9}
    assert {k: P(3, 1300, 72, 33)[k] for k in ("bwd_form", "bwd_gz", "bwd_tiles", "bwd_wgs", "bwd_wgs_launched")} == \
        {"bwd_form": "uni32", "bwd_gz": 4, "bwd_tiles": 6, "bwd_wgs": 36, "bwd_wgs_launched": 48}
    assert P(3, 1300, 72, 87)["bwd_form"] == "uni64" and P(100, 600, 64, 87)["nset"] == 2
    F = lambda T, C, k: D.plan_of(D.Case("q", "f32", 2, T, C, k, 1, "int", ""))["ts"]
    assert [F(128, 4, k) for k in (39, 41, 63, 65)] == [3, 2, 2, 1]
