"""The BiLSTM context kernels (csrc/lstm.hip, csrc/lstm_body.h) called directly through lasr_bilstm_fwd / lasr_bilstm_bwd and
compared with the f64 per-utterance loop of tests/helpers/bilstm_ref.py (itself checked against torch.nn.LSTM in
tests/test_host_bilstm_ref.py), plus the two small kernels of the same path: lasr_copy_cols and lasr_colsum_f32.

Inputs are seeded (helpers/bilstm_ref.py make_inputs): gx ~ N(0, 1), W_hh and the biases uniform in +-1/sqrt(40), dout ~ N(0, 1).
Relative L2 is taken per utterance and per direction over t < len (worst_per_utterance), dW_hh per direction and per call.

Gates.  Ceilings are the project's f32 per-unit gates (tests/test_gpu_units.py TOL["f32"]): out and saved 5e-6, dg and dW_hh 2e-5.
Each gate is min(ceiling, 2 x the worst value measured on the MI355X) - the kernels are deterministic and the seeds fixed, the
factor covers a future legitimate reordering of f32 sums and nothing else.  Measured values and the reference's own f32-vs-f64
floor on the same cases: profiles/lstm_op_parity.json ("measured_mi355x", "cpu_f32_floor"); the table below quotes them.

| record (lstm_op_*)        | floor (CPU f32) | measured MI355X | gate |
|---|---|---|---|
| colsum_16032x28_colsum | - | 8.04e-08 | 1.61e-07 |
| colsum_1608x160_colsum | - | 6.50e-08 | 1.30e-07 |
| colsum_17x160_colsum | - | 5.54e-08 | 1.11e-07 |
| colsum_1x160_colsum | - | 0.00e+00 | 0.00e+00 |
| colsum_300x4334_colsum | - | 1.14e-07 | 2.28e-07 |
| colsum_5x257_colsum | - | 5.09e-08 | 1.02e-07 |
| edges_batched_dwhh | 3.5e-07 | 2.38e-07 | 4.77e-07 |
| edges_dg | 1.2e-07 | 1.88e-07 | 3.75e-07 |
| edges_out | 9.4e-08 | 2.00e-07 | 3.99e-07 |
| edges_saved | 9.4e-08 | 2.00e-07 | 3.99e-07 |
| long_2001_dg | 1.1e-07 | 1.61e-07 | 3.22e-07 |
| long_2001_dwhh | 8.3e-07 | 3.14e-07 | 6.29e-07 |
| long_2001_out | 8.7e-08 | 1.78e-07 | 3.56e-07 |
| long_2001_saved | 8.7e-08 | 1.78e-07 | 3.56e-07 |
| long_801_501_dg | 1.1e-07 | 1.63e-07 | 3.27e-07 |
| long_801_501_dwhh | 6.8e-07 | 2.56e-07 | 5.13e-07 |
| long_801_501_out | 8.7e-08 | 1.80e-07 | 3.60e-07 |
| long_801_501_saved | 8.7e-08 | 1.80e-07 | 3.60e-07 |
| per_length_dwhh | 1.8e-07 | 2.55e-07 | 5.11e-07 |
| saturated_dg | 2.3e-07 | 3.67e-07 | 7.35e-07 |
| saturated_out | 6.9e-08 | 1.12e-07 | 2.24e-07 |
"""
import math
import os
import sys

import pytest
import torch

from conftest import record_measured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bilstm_ref as L  # noqa: E402

pytestmark = pytest.mark.gpu

H, G = L.H, L.G
CEIL = {"out": 5e-6, "saved": 5e-6, "dg": 2e-5, "dwhh": 2e-5, "colsum": 2e-6}
# worst values measured on the MI355X (profiles/lstm_op_parity.json "measured_mi355x"); a record without one is held to its ceiling
MEASURED = {
    "colsum_16032x28_colsum": 8.039e-08,
    "colsum_1608x160_colsum": 6.504e-08,
    "colsum_17x160_colsum": 5.537e-08,
    "colsum_1x160_colsum": 0.000e+00,
    "colsum_300x4334_colsum": 1.141e-07,
    "colsum_5x257_colsum": 5.094e-08,
    "edges_batched_dwhh": 2.383e-07,
    "edges_dg": 1.877e-07,
    "edges_out": 1.996e-07,
    "edges_saved": 1.996e-07,
    "long_2001_dg": 1.608e-07,
    "long_2001_dwhh": 3.143e-07,
    "long_2001_out": 1.780e-07,
    "long_2001_saved": 1.780e-07,
    "long_801_501_dg": 1.633e-07,
    "long_801_501_dwhh": 2.563e-07,
    "long_801_501_out": 1.801e-07,
    "long_801_501_saved": 1.801e-07,
    "per_length_dwhh": 2.553e-07,
    "saturated_dg": 3.674e-07,
    "saturated_out": 1.122e-07,
}


def _gate(name):
    ceil = CEIL[name.rsplit("_", 1)[1]]
    return min(ceil, 2.0 * MEASURED[name]) if name in MEASURED else ceil


def _check(name, value):
    """print and record the figure, then hold it to min(ceiling, 2 x measured) (<=: a measured 0 - the one-row column sum - is
    held to exactly 0).  A NaN fails: the comparators propagate it (helpers/bilstm_ref.py worst_of)."""
    assert math.isfinite(value), (name, value)
    gate = _gate(name)
    print("lstm_op_%s = %.3e (gate %.3e)" % (name, value, gate))
    record_measured("lstm_op_" + name, value)
    assert value <= gate, (name, value, gate)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run(dev, name, **kw):
    inp, lens = L.case(name)
    dout = kw.pop("dout", inp["dout"])
    return L.bilstm_gpu(dev, inp["gx_f"], inp["gx_r"], inp["whh"], inp["bias_ih"], inp["bias_hh"], lens, dout, **kw)


def _saved_worst(got, ref, lens):
    s = L.split_saved(got["saved"])
    return L.worst_of(L.worst_per_utterance(s, ref, lens, q) for q in ("gates", "c", "h"))


def _dwhh_worst(got, ref):
    return L.worst_of(L.rel_l2(got["dwhh"][d], ref["dwhh"][d]) for d in range(2))


def _assert_written(got, lens):
    """the NaN / sentinel prefills are gone where the kernels have to write: out, saved and dg finite over t < len, out and dg
    exactly 0 over t >= len, dW_hh finite everywhere"""
    for b, n in enumerate(lens):
        n = min(int(n), got["out"].shape[1])
        assert bool((got["out"][b, n:] == 0).all()), ("out not zero past len", b, n)
        assert bool((got["dg"][:, b, n:] == 0).all()), ("dg not zero past len", b, n)
        assert bool(torch.isfinite(got["out"][b, :n]).all()), ("out", b, n)
        assert bool(torch.isfinite(got["saved"][b, :n]).all()), ("saved", b, n)
        assert bool(torch.isfinite(got["dg"][:, b, :n]).all()), ("dg", b, n)
    assert bool(torch.isfinite(got["dwhh"]).all()), "dwhh"


_EDGE_RUN = {}


def _edge_run(dev):
    """the edge-length call (ld = 96, col0 = 8, NaN in every d(out) column outside the window), run once per process"""
    if "r" not in _EDGE_RUN:
        _EDGE_RUN["r"] = _run(dev, "edges", ld=96, col0=8, dout_pad=float("nan"))
    return _EDGE_RUN["r"]


def test_bilstm_length_edges_f32(dev):
    """One call, T = 36, the 17 lengths 0, 1, 2, 7, 8, 9, 15 .. 18, 23 .. 25, 31 .. 34, output window ld = 96 / col0 = 8.
    Pins, per utterance: the split of the steps into len % 8 odd steps plus whole rounds of the 8-deep register ring in both
    kernels (len % 8 = 0, 1, 7 at one, two, three and four rounds; a wrong split shifts every operand of a round), the clamped
    priming and refill loads at len < 8 and len = 0 (the length-0 utterance loads row 0 and must use nothing of it), the reverse
    direction's start at len - 1, the zero fill of `out` and `dg` over the padded frames (NaN / sentinel prefill: a frame that is
    not written shows), and the column window of the output store and of the d(out) load (sentinel outside, NaN d(out) outside).
    d(out) rows at t >= len hold NaN in a second run: the results must not change by a bit (the fetches clamp t into
    [0, len - 1])."""
    inp, lens = L.case("edges")
    ref = L.case_ref("edges")
    got = _edge_run(dev)
    B, T = len(lens), L.EDGE_T
    full = got["out_full"]
    assert bool((full[:, :, :8] == L.OUT_SENTINEL).all()) and bool((full[:, :, 88:] == L.OUT_SENTINEL).all())
    _assert_written(got, lens)
    _check("edges_out", L.worst_per_utterance(got, ref, lens, "out"))
    _check("edges_saved", _saved_worst(got, ref, lens))
    _check("edges_dg", L.worst_per_utterance(got, ref, lens, "dg"))
    dnan = inp["dout"].clone()
    for b, n in enumerate(lens):
        dnan[b, n:] = float("nan")
    got2 = _run(dev, "edges", ld=96, col0=8, dout_pad=float("nan"), dout=dnan)
    for k in ("out_full", "saved", "dg", "dwhh"):
        assert _same_bits(got[k], got2[k]), ("d(out) rows past len changed " + k)


def test_bilstm_dwhh_per_length(dev):
    """Each of the 17 lengths as its own B = 1 call (T = len + 2), so that dW_hh is ONE utterance's sum: bilstm_dwhh_kernel cuts
    the len - 1 steps that have a previous state into kDwZ * kDwSlices = 16 parts of per = ceil((len - 1) / 16) steps.  In this table: per = 1 up to len 17 (len - 1 parts of one
    step, the rest empty; all 16 in use at len 17), per = 2 at 18 .. 33 (a ragged last part of one step at len 18, 24 and 32,
    empty parts behind it; 16 full parts at len 33), per = 3 at len 34 (11 full parts, 5 empty).  A part that starts one step off,
    takes h(t) for h(t -+ 1), or counts the first step (which has no previous state) moves one utterance's dW_hh by percent; a
    partial that an empty part leaves unwritten is NaN from the prefilled workspace; lengths 0 and 1 must give exactly 0."""
    errs = []
    for n in L.EDGE_LENS:
        name = "len%d" % n
        got = _run(dev, name)
        _assert_written(got, [n])
        if n <= 1:
            assert bool((got["dwhh"] == 0).all()), n
            continue
        e = _dwhh_worst(got, L.case_ref(name))
        print("len %d: dW_hh rel L2 %.3e" % (n, e))
        errs.append(e)
    _check("per_length_dwhh", L.worst_of(errs))


def test_bilstm_batched_dwhh_is_the_sum(dev):
    """dW_hh of the whole 17-utterance call against the f64 sum over the batch: the reduction over B * kDwZ = 68 partials per
    direction (launch_reduce_partials) at a B that is not a multiple of 8, and the [2][B * kDwZ] row order of the partials."""
    _check("edges_batched_dwhh", _dwhh_worst(_edge_run(dev), L.case_ref("edges")))


@pytest.mark.parametrize("name", ["long_801_501", "long_2001"])
def test_bilstm_long_recurrence_f32(dev, name):
    """801 / 501 and 2001 dependent steps (the 40 s clip) in f32 against f64, forward and backward, at the f32 gates - what the
    whole-model tests compare only at the bf16 unit gates.  An error that grows with the step count (a drifting cell state, the
    v_exp_f32 / v_rcp_f32 non-linearities feeding back) shows here and nowhere shorter."""
    _, lens = L.case(name)
    ref = L.case_ref(name)
    got = _run(dev, name)
    _assert_written(got, lens)
    _check(name + "_out", L.worst_per_utterance(got, ref, lens, "out"))
    _check(name + "_saved", _saved_worst(got, ref, lens))
    _check(name + "_dg", L.worst_per_utterance(got, ref, lens, "dg"))
    _check(name + "_dwhh", _dwhh_worst(got, ref))


def test_bilstm_saturated_gates(dev):
    """gx scaled by 12 (pre-activations to about +-40) and +-1e4 in eight entries: __expf overflows to inf inside sigmoid_fast /
    tanh_fast and v_rcp_f32(inf) must come back as 0, not NaN; i(1 - i), 1 - g^2 and 1 - tanh(c)^2 are formed from gates at 0 and 1.
    Everything stays finite, out at the activation gate, dg at the gradient gate."""
    _, lens = L.case("saturated")
    ref = L.case_ref("saturated")
    got = _run(dev, "saturated")
    _assert_written(got, lens)
    _check("saturated_out", L.worst_per_utterance(got, ref, lens, "out"))
    _check("saturated_dg", L.worst_per_utterance(got, ref, lens, "dg"))


@pytest.mark.parametrize("name,T,ld,col0", [("edges", L.EDGE_T, 96, 8), ("len501", 503, 80, 0)])
def test_bilstm_bf16_store_and_load_are_exact(dev, name, T, ld, col0):
    """The bf16 instantiations differ from the f32 ones in one store and one load.  Forward: the bf16 output is the f32 output
    rounded to nearest even, bit for bit, and `saved` does not depend on the output type.  Backward: a bf16 d(out) (a zero-
    extending 16-bit load widened by a shift at use, lstm_body.h) gives the bits of the same values passed as f32, on the same
    `saved`, in dg and dW_hh."""
    inp, lens = L.case(name)
    a = (inp["gx_f"], inp["gx_r"], inp["whh"], inp["bias_ih"], inp["bias_hh"], lens)
    out32, saved32 = L.bilstm_gpu_fwd(dev, *a, ld=ld, col0=col0, dtype=torch.float32)
    out16, saved16 = L.bilstm_gpu_fwd(dev, *a, ld=ld, col0=col0, dtype=torch.bfloat16)
    assert _same_bits(out16.cpu(), out32.cpu().bfloat16())             # (the sentinel is a bf16 value: the whole tensor compares)
    assert _same_bits(saved16.cpu(), saved32.cpu())
    d16 = torch.full((len(lens), T, ld), float("nan"), dtype=torch.bfloat16)
    d16[:, :, col0:col0 + 2 * H] = inp["dout"].bfloat16()
    r16 = L.bilstm_gpu_bwd(dev, d16, inp["whh"], lens, saved32, ld, col0)
    r32 = L.bilstm_gpu_bwd(dev, d16.float(), inp["whh"], lens, saved32, ld, col0)
    for x16, x32, k in zip(r16, r32, ("dg_f", "dg_r", "dwhh_f", "dwhh_r")):
        assert bool(torch.isfinite(x16).all()), k
        assert _same_bits(x16.cpu(), x32.cpu()), k


def test_bilstm_len_above_T_clamps_and_is_deterministic(dev):
    """lens[b] > T is clamped to T in all three kernels (forward, backward, dW_hh): [T + 5, T, 3] gives the bits of [T, T, 3] -
    without the clamp the reverse direction would start five frames past the utterance's rows.  A repeated call gives the same
    bits (fixed-order sums everywhere)."""
    T = 12
    inp = L.make_inputs(3, T, seed=77)
    a = (inp["gx_f"], inp["gx_r"], inp["whh"], inp["bias_ih"], inp["bias_hh"])
    r0 = L.bilstm_gpu(dev, *a, [T, T, 3], inp["dout"])
    r1 = L.bilstm_gpu(dev, *a, [T + 5, T, 3], inp["dout"])
    r2 = L.bilstm_gpu(dev, *a, [T + 5, T, 3], inp["dout"])
    assert bool(torch.isfinite(r0["dwhh"]).all()) and bool((r0["dwhh"] != 0).any())
    for k in ("out_full", "saved", "dg", "dwhh"):
        assert _same_bits(r0[k], r1[k]), ("clamp", k)
        assert _same_bits(r1[k], r2[k]), ("repeat", k)


# ---- the two small kernels of the same path ----

@pytest.mark.parametrize("rows,ncols", [(1, 160), (37, 80), (4200, 256)])
def test_copy_cols_against_indexing(dev, rows, ncols):
    """lasr_copy_cols (the cat() of the context branch, its backward slice, the bias-gradient copy) against plain indexing: all
    four dtype pairs, accumulate 0 and 1, non-zero column offsets in leading dimensions wider than the window, guard columns
    untouched.  f32 -> bf16 is .bfloat16() bit for bit, bf16 -> f32 is exact, accumulate adds in f32 and rounds once.
    (4200, 256) is 1 075 200 elements: past the 4096 x 256 grid cap, so the grid-stride loop wraps."""
    from lightning_asr_amd import _lib
    from lightning_asr_amd.ops import _p, _stream
    code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}
    g = torch.Generator().manual_seed(rows * 31 + ncols)
    scol0, dcol0 = 3, 5
    lds, ldd = scol0 + ncols + 4, dcol0 + ncols + 7
    for sdt in (torch.float32, torch.bfloat16):
        for ddt in (torch.float32, torch.bfloat16):
            for acc in (0, 1):
                src = torch.randn(rows, lds, generator=g).to(sdt)
                dst0 = torch.randn(rows, ldd, generator=g).to(ddt)
                src_d, dst_d = src.to(dev), dst0.to(dev)
                _lib.call("lasr_copy_cols", _p(src_d), code[sdt], lds, scol0, _p(dst_d), code[ddt], ldd, dcol0, rows, ncols, acc,
                          _stream())
                torch.cuda.synchronize()
                want = dst0.clone()
                v = src[:, scol0:scol0 + ncols].float()
                if acc:
                    v = v + dst0[:, dcol0:dcol0 + ncols].float()
                want[:, dcol0:dcol0 + ncols] = v.to(ddt)
                assert _same_bits(dst_d.cpu(), want), (sdt, ddt, acc)


@pytest.mark.parametrize("rows,C", [(1, 160), (17, 160), (1608, 160), (16032, 28), (300, 4334), (5, 257)])
def test_colsum_against_f64(dev, rows, C):
    """lasr_colsum_f32 (the bias gradients of the separate BiLSTM path, the decoder bias) against an f64 column sum with a workspace
    of exactly lasr_colsum_workspace_bytes: one row, a ragged last slab of the 32-row and of the 256-row form, 28 columns dealt over
    9 row lanes, a second column chunk of one column (257).  The second stage sums in f64 in a fixed order, so the only error is
    the f32 partial of one slab.  One byte less of workspace is refused before anything is launched."""
    from lightning_asr_amd import _lib
    from lightning_asr_amd.ops import _p, _stream
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g)
    x_d = x.to(dev)
    nb = int(_lib.load().lasr_colsum_workspace_bytes(rows, C))
    assert nb > 0 and nb % 4 == 0
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((C,), float("nan"), dtype=torch.float32, device=dev)
    with pytest.raises(_lib.LasrError, match="workspace"):
        _lib.call("lasr_colsum_f32", _p(x_d), _p(out), rows, C, _p(ws), nb - 1, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    _lib.call("lasr_colsum_f32", _p(x_d), _p(out), rows, C, _p(ws), nb, _stream())
    torch.cuda.synchronize()
    e = L.rel_l2(out.cpu(), x.double().sum(0))
    if rows == 1:
        assert torch.equal(out.cpu(), x[0])
    _check("colsum_%dx%d_colsum" % (rows, C), e)
