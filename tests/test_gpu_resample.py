"""GPU tier of the resampler kernel (csrc/resample.hip) against the numpy f64 oracle (tests/helpers/resample_oracle.py).

Gates are derived, not measured.  The oracle is run in f64 on the kernel's own operands - the bank's f32 taps and the f32 (or
PCM16 / 32768) inputs - so what is left is the kernel's f32 accumulation: `taps` fused multiply-adds, each within half an ulp of
a partial sum bounded by A = sum_k |h x|, i.e. |out - y| <= (taps + 1) 2^-24 A per sample (a CPU f32 emulation stayed under 0.26
of it).  PCM16 output adds the rounding to an integer: |out - 32768 y| <= 0.5 + 32768 (taps + 1) 2^-24 A, with 32768 y clamped to
[-32768, 32767] as the operator clamps it (white noise at +-0.9 does overshoot +-1 after interpolation; the clamp moves two values
no further apart than they were, so the bound holds for the clamped pair).

Row lengths per conversion: 0, 1, width - 1, 4001, the three that put n_out at tile - 1, tile, tile + 1 for the kernel's own output
tile (where up / down cannot reach a value, the next n_out above it), and 2 tile + 3."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

CONVERSIONS = [(44100, 16000), (22050, 16000), (48000, 16000), (8000, 16000), (9, 10), (11, 10)]
LEAD = 1 << 30
CANARY = {torch.float32: 123.0, torch.int16: 12345}
DTYPES = {"f32": torch.float32, "pcm16": torch.int16}
_cache = {}


def _resampler(key, convs, dev):
    from lightning_asr_amd import ops
    if key not in _cache:
        _cache[key] = ops.Resampler(convs, dev)
    return _cache[key]


def _bank_taps(rs, i):
    """(up, taps) f32 taps of conversion i as the kernel reads them"""
    img = rs.bank.cpu().numpy()
    up, down, width, taps, offset = [int(v) for v in img[16 + 8 * i:21 + 8 * i]]
    return img.view(np.float32)[offset:offset + up * taps].reshape(taps, up).T.astype(np.float64)


def _n_in_for(n_out_target, up, down):
    """the smallest n_in whose n_out is >= the target"""
    n = max(0, (n_out_target * down) // up - 2)
    while O.out_len(n, up, down) < n_out_target:
        n += 1
    return n


def _lengths(rs, i):
    up, down, width, _ = O.geometry(*CONVERSIONS[i])
    tile = rs.tile(i)
    assert tile % up == 0 and 0 < tile <= 1024
    return [0, 1, width - 1, 4001] + [_n_in_for(t, up, down) for t in (tile - 1, tile, tile + 1, 2 * tile + 3)]


def _case(dev, i, n, in_name):
    """inputs of (conversion i, n samples, input dtype) and the oracle on them: computed once, shared by the alone and mixed launches"""
    key = ("case", i, n, in_name)
    if key not in _cache:
        full = _resampler("all", CONVERSIONS, dev)
        rng = np.random.RandomState(1000 * i + n % 997 + (7 if in_name == "pcm16" else 0))
        x = rng.uniform(-0.9, 0.9, n).astype(np.float32)
        if in_name == "pcm16":
            x = np.rint(x * 32768.0).astype(np.int16)
            xr = x.astype(np.float64) / 32768.0
        else:
            xr = x.astype(np.float64)
        y, a = O.resample(xr, *CONVERSIONS[i], h=_bank_taps(full, i))
        _cache[key] = (x, y, a)
    return _cache[key]


def _launch_and_check(dev, rs, rows, in_name, out_name):
    """rows: [(conversion index in CONVERSIONS, conversion index in rs, n_in)] - one launch, every property of the contract"""
    in_dt, out_dt = DTYPES[in_name], DTYPES[out_name]
    B = len(rows)
    cases = [_case(dev, i, n, in_name) for i, _, n in rows]
    L = max(max(n for _, _, n in rows), 1)
    n_outs = [c[1].size for c in cases]
    L_out = max(n_outs) + 3
    garbage = 0.77 if in_dt == torch.float32 else 25000
    host = torch.full((B, L + 7), garbage, dtype=in_dt)                 # in_pitch > L; whatever lies past a row's length is never read
    for b, (x, _, _) in enumerate(cases):
        host[b, :x.size] = torch.from_numpy(x)
    wave = host.to(dev)[:, :L]
    lens = torch.tensor([n for _, _, n in rows], dtype=torch.int32, device=dev)
    ids = torch.tensor([j for _, j, _ in rows], dtype=torch.int32, device=dev)
    buf = torch.full((B, L_out + 5), CANARY[out_dt], dtype=out_dt, device=dev)      # out_pitch > L_out, canary past L_out
    out, out_lens = rs(wave, lens, ids if len(rs.factors) > 1 else None, out_dtype=out_dt, out=buf, L_out=L_out)
    torch.cuda.synchronize()
    assert out_lens.cpu().tolist() == n_outs
    res = buf.cpu().numpy()
    assert (res[:, L_out:] == CANARY[out_dt]).all(), "canary past L_out"
    for b, ((i, _, n), (_, y, a)) in enumerate(zip(rows, cases)):
        taps = O.geometry(*CONVERSIONS[i])[3]
        got = res[b, :y.size].astype(np.float64)
        assert (res[b, y.size:L_out] == 0).all(), ("zero fill", CONVERSIONS[i], n)
        bound = (taps + 1) * 2.0 ** -24 * a
        if out_dt == torch.int16:
            err, bound = np.abs(got - np.clip(32768.0 * y, -32768.0, 32767.0)), 0.5 + 32768.0 * bound
        else:
            err = np.abs(got - y)
        if y.size:
            worst = float((err / np.maximum(bound, 1e-300)).max())
            print("resample %s->%s %s n=%d: worst |err| / bound = %.3f" % (in_name, out_name, CONVERSIONS[i], n, worst))
            assert (err <= bound).all(), (CONVERSIONS[i], n, in_name, out_name, worst)


@pytest.mark.parametrize("out_name", ["f32", "pcm16"])
@pytest.mark.parametrize("in_name", ["f32", "pcm16"])
def test_parity_one_conversion_per_launch(dev, in_name, out_name):
    full = _resampler("all", CONVERSIONS, dev)
    for i, conv in enumerate(CONVERSIONS):
        rs = _resampler(("one", i), [conv], dev)
        assert np.array_equal(_bank_taps(rs, 0), _bank_taps(full, i))
        ls = _lengths(full, i)
        for part in (ls[:4], ls[4:]):                                    # B = 4
            _launch_and_check(dev, rs, [(i, 0, n) for n in part], in_name, out_name)


@pytest.mark.parametrize("out_name", ["f32", "pcm16"])
@pytest.mark.parametrize("in_name", ["f32", "pcm16"])
def test_parity_mixed_conversions_in_one_launch(dev, in_name, out_name):
    full = _resampler("all", CONVERSIONS, dev)
    pairs = [(i, n) for i in range(len(CONVERSIONS)) for n in _lengths(full, i)]
    # deal the (conversion, length) pairs so that every launch of 4 rows mixes 4 different conversions
    order = sorted(range(len(pairs)), key=lambda k: (k % 8, k // 8))
    pairs = [pairs[k] for k in order]
    for s in range(0, len(pairs), 4):
        rows = [(i, i, n) for i, n in pairs[s:s + 4]]
        assert len(set(i for i, _, _ in rows)) == len(rows)
        _launch_and_check(dev, full, rows, in_name, out_name)


def test_pcm16_output_saturates(dev):
    """a full-scale square wave overshoots +-1 after interpolation (Gibbs): those samples are exactly 32767 / -32768, never wrapped"""
    from lightning_asr_amd import ops
    period = 16
    pcm = np.where((np.arange(640) // (period // 2)) % 2 == 0, 32767, -32767).astype(np.int16)
    rs = _resampler(("one", 3), [(8000, 16000)], dev)
    h = _bank_taps(rs, 0)
    y, a = O.resample(pcm.astype(np.float64) / 32768.0, 8000, 16000, h=h)
    slack = 0.5 + 32768.0 * (15 + 1) * 2.0 ** -24 * a
    over, under = 32768.0 * y > 32767.5 + slack, 32768.0 * y < -32768.5 - slack
    assert y.max() > 1.0 and y.min() < -1.0 and over.sum() > 10 and under.sum() > 10      # the oracle does leave [-1, 1]
    for in_dt in (torch.int16, torch.float32):
        x = torch.from_numpy(pcm) if in_dt == torch.int16 else torch.from_numpy(pcm.astype(np.float32) / 32768.0)
        out, n = rs(x.to(dev).unsqueeze(0), out_dtype=torch.int16)
        got = out.cpu().numpy()[0].astype(np.float64)
        assert int(n[0]) == y.size == 1280
        assert (got[over] == 32767).all() and (got[under] == -32768).all()
        assert (np.abs(got - np.clip(32768.0 * y, -32768, 32767)) <= slack).all()
    out2, _ = ops.resample(torch.from_numpy(pcm).to(dev), 8000, 16000)              # the convenience wrapper: same kernel, int16 -> int16
    assert out2.dtype == torch.int16 and np.array_equal(out2.cpu().numpy().astype(np.float64), got)


def test_identity_rows_are_copied_bit_for_bit(dev):
    rs = _resampler("ident", [(16000, 16000), (8000, 16000), (44100, 44100)], dev)
    assert rs.factors == [(1, 1), (2, 1), (1, 1)]
    g = torch.Generator().manual_seed(3)
    n = [2051, 0, 700, 1]
    # f32: arbitrary bit patterns short of NaN (denormals, -0.0, huge values) survive
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (4, 2060), generator=g, dtype=torch.int64).to(torch.int32)
    xf = bits.view(torch.float32)
    xf = torch.where(torch.isnan(xf), torch.zeros_like(xf), xf)
    xf[0, :3] = torch.tensor([-0.0, 1e-42, -3e38])
    xi = torch.randint(-32768, 32768, (4, 2060), generator=g, dtype=torch.int64).to(torch.int16)
    xi[0, :2] = torch.tensor([-32768, 32767], dtype=torch.int16)
    lens = torch.tensor([n[0], n[1], n[2] | LEAD, n[3]], dtype=torch.int32)          # row 2 carries a lead-in sample: 701 samples in the row
    copied = [n[0], n[1], n[2] + 1, n[3]]
    ids = torch.tensor([0, 2, 0, 2], dtype=torch.int32)
    for x in (xf, xi):
        buf = torch.full((4, 2070), CANARY[x.dtype], dtype=x.dtype, device=dev)
        out, out_lens = rs(x.to(dev), lens.to(dev), ids.to(dev), out=buf, L_out=2060)
        torch.cuda.synchronize()
        assert torch.equal(out_lens.cpu(), lens)                                     # the flag passes through
        res = buf.cpu()
        assert (res[:, 2060:] == CANARY[x.dtype]).all()
        for b in range(4):
            assert torch.equal(res[b, :copied[b]].view(torch.int32 if x.dtype == torch.float32 else torch.int16),
                               x[b, :copied[b]].view(torch.int32 if x.dtype == torch.float32 else torch.int16)), b
            assert (res[b, copied[b]:2060] == 0).all()
    # dtypes differ: only the scale (and the rounding) apply
    out, _ = rs(xi.to(dev), lens.to(dev), ids.to(dev), out_dtype=torch.float32)
    assert torch.equal(out.cpu()[0, :n[0]], xi[0, :n[0]].float() / 32768.0)
    small = (torch.rand(4, 2060, generator=g) * 2.2 - 1.1)
    out, _ = rs(small.to(dev), lens.to(dev), ids.to(dev), out_dtype=torch.int16)
    want = torch.clamp(torch.round(small.double() * 32768.0), -32768, 32767).to(torch.int16)      # round half to even, as rint
    assert torch.equal(out.cpu()[0, :n[0]], want[0, :n[0]])
    # identity and filtered rows side by side
    ids2 = torch.tensor([0, 1, 0, 1], dtype=torch.int32)
    lens2 = torch.tensor([2051, 900, 700 | LEAD, 33], dtype=torch.int32)
    out, out_lens = rs(xi.to(dev), lens2.to(dev), ids2.to(dev))
    assert out_lens.cpu().tolist() == [2051, 1800, 700 | LEAD, 66]
    assert torch.equal(out.cpu()[2, :701], xi[2, :701])
    y, a = O.resample(xi[1, :900].double().numpy() / 32768.0, 8000, 16000, h=_bank_taps(rs, 1))
    assert (np.abs(out.cpu()[1, :1800].double().numpy() - np.clip(32768.0 * y, -32768, 32767)) <= 0.5 + 32768.0 * 16 * 2.0 ** -24 * a).all()


def test_bad_bank_or_conversion_gives_empty_rows_and_errors_are_refused(dev):
    from lightning_asr_amd import _lib, ops
    rs = _resampler(("one", 3), [(8000, 16000)], dev)
    x = torch.rand(2, 100, device=dev)
    out, n = rs(x, conv_id=torch.tensor([0, 5], dtype=torch.int32, device=dev))
    assert n.cpu().tolist() == [200, 0] and not out[1].any() and out[0].any()
    with pytest.raises(_lib.LasrError):
        rs(x.cpu())
    with pytest.raises(_lib.LasrError):
        rs(x.double())
    with pytest.raises(_lib.LasrError):
        rs(x, out=torch.empty(2, 10, device=dev), L_out=200)
    with pytest.raises(_lib.LasrError):
        ops.Resampler([(8000, 16000)] * 9, dev)
    with pytest.raises(_lib.LasrError):
        ops.Resampler([(44101, 16000)], dev)


def test_resample_in_a_captured_graph(dev):
    rs = _resampler("all", CONVERSIONS, dev)
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(4, 3000, generator=g) - 0.5).to(dev)
    lens = torch.tensor([3000, 1234, 0, 2999], dtype=torch.int32, device=dev)
    ids = torch.tensor([0, 4, 2, 5], dtype=torch.int32, device=dev)
    a = rs(x, lens, ids)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rs(x, lens, ids)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = rs(x, lens, ids)
    for _ in range(2):
        for o in c:
            o.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(a, c):
            assert torch.equal(u, v)
