"""GPU tier of the noise and reverberation kernels (csrc/wave_aug.hip) against the numpy f64 oracle (tests/helpers/wave_aug_oracle.py).

Gates are derived, not measured.  The oracle runs in f64 on the kernel's own operands (the bank's f32 taps, the f32 or PCM16 / 32768
inputs, the PCM16 / 32768 noise), so what is left is the kernel's f32 arithmetic:
  energies  E_x, E_n: f64 sums of exact products, 1e-9 relative.
  FIR       K fused multiply-adds, each within half an ulp of a partial sum bounded by A_j = sum_k |h x|:  e_j = (K + 1) 2^-24 A_j;
            E_y within 2 |e| sqrt(E_y) + 1e-9 E_y  (|y + e|^2 - |y|^2 <= 2 |y| |e| + |e|^2, and |e| is far below |y|: asserted).
  output    against g_s y_ref + g_n v with the gains formed from the RETURNED (already checked) stats: g_s e_j for the FIR, and
            2^-22 (|g_s y_j| + |g_n v_j|) for the two products, the sum and the gains' own rounding (device sqrt / pow against numpy).
  PCM16     0.5 + 32768 * bound against the reference clamped to [-32768, 32767], as the operator clamps it.
The worst-case FIR bound is loose at long K, so a second gate holds the kernel's largest FIR error per row (read from the
workspace's y) to 4 x that of an ascending-order numpy-f32 emulation of the same row - the factor covers fma against separate
rounding - floored at 2^-24 max A.  The RIRs are decaying noise (time constant K / 7) so that e_j stays under 2 % of the row's RMS:
asserted on the inputs.

Shapes come from the kernel's own tile and chunk: n in {1, tile - 1, tile, tile + 1, 2 tile + 5} x K in {1, 2, chunk - 1, chunk,
chunk + 1, 2 chunk + 3} x d in {0, K // 2, K - 1}; noise clips of 1 sample, shorter than the rows (several wraps) and longer, starts
at 0, in the middle and at len - 1; reverb-only, noise-only, both and neither in ONE launch; all four dtype pairs; `out` aliased
and separate; an f32 noise bank."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import wave_aug_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

LEAD = 1 << 30
CANARY = {torch.float32: 123.0, torch.int16: 12345}
DTYPES = {"f32": torch.float32, "pcm16": torch.int16}
NOISE_LENS = [1, 777, 5003]
_cache = {}


def make_rir(K, d, seed):
    """decaying noise of exactly K taps with its peak at d: the last tap is large enough for the builder to keep it"""
    rng = np.random.RandomState(seed)
    h = rng.standard_normal(K) * np.exp(-np.arange(K) / (K / 7.0))
    peak = 2.0 * np.abs(h).max() + 1.0
    if K - 1 != d:
        h[K - 1] = 0.01 * peak
    h[d] = peak
    return (h / peak * 0.5).astype(np.float32)


def _setup(dev):
    """the banks, the rows and the inputs of the parity launches: built once"""
    if "setup" in _cache:
        return _cache["setup"]
    from lightning_asr_amd import ops
    tile, chunk = ops.wave_augment_tile(), ops.wave_augment_chunk()
    assert tile >= 64 and chunk >= 16
    ns = [1, tile - 1, tile, tile + 1, 2 * tile + 5]
    geo = []
    for K in (1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk + 3):
        for d in sorted({0, K // 2, K - 1}):
            geo.append((K, d))
    rirs = [make_rir(K, d, 100 + i) for i, (K, d) in enumerate(geo)]
    rng = np.random.RandomState(5)
    noises = [np.rint(rng.uniform(-0.5, 0.5, m) * 32768.0).astype(np.int16) for m in NOISE_LENS]
    aug = ops.WaveAugmenter(rirs, noises, dev)
    assert list(zip(aug.rir_taps, aug.rir_delay)) == geo, "the builder keeps the RIRs as the test made them"
    rows = []                                            # (n, rir, noise, start, snr_cdb)
    for n in ns:
        for r in range(len(geo)):
            rows.append((n, r, -1, 0, 0))                # reverb only: the FIR sweep
    k = 0
    for n in ns:
        for c, m in enumerate(NOISE_LENS):
            for start in sorted({0, m // 2, m - 1}):
                both = k % 2 == 1
                rows.append((n, (3 * k) % len(geo) if both else -1, c, start, 500 + 173 * (k % 9)))      # 5 .. 19 dB
                k += 1
        rows.append((n, -1, -1, 0, 0))                   # neither
    L = max(ns)
    xs = {}
    x32 = np.random.RandomState(9).uniform(-0.9, 0.9, (len(rows), L)).astype(np.float32)
    xs["f32"] = x32
    xs["pcm16"] = np.rint(x32 * 32768.0).astype(np.int16)
    _cache["setup"] = dict(aug=aug, rirs=rirs, geo=geo, noises=noises, rows=rows, L=L, xs=xs, ns=ns)
    return _cache["setup"]


def _reference(dev, in_name):
    """the oracle on every row of the parity launch for one input dtype: computed once, never modified"""
    key = ("ref", in_name)
    if key not in _cache:
        s = _setup(dev)
        img = s["aug"].rir_bank.cpu().numpy()
        refs = []
        for b, (n, r, c, start, snr) in enumerate(s["rows"]):
            x = s["xs"][in_name][b, :n].astype(np.float64) / (32768.0 if in_name == "pcm16" else 1.0)
            h = d = None
            if r >= 0:
                K, d, off = [int(v) for v in img[4 + 4 * r:7 + 4 * r]]
                h = img.view(np.float32)[off:off + K].astype(np.float64)
                assert np.array_equal(h, s["rirs"][r].astype(np.float64))
            clip = s["noises"][c].astype(np.float64) / 32768.0 if c >= 0 else None
            ref = O.augment(x, h, d or 0, clip, start, snr)
            ref["K"] = h.size if h is not None else 0
            ref["e"] = (ref["K"] + 1) * 2.0 ** -24 * ref["A"] if h is not None else np.zeros(n)
            if h is not None:                            # the issue's condition on the inputs: e_j under 2 % of the row's RMS
                assert ref["e"].max() <= 0.02 * np.sqrt(ref["stats"][1] / n), (b, n, ref["K"])
            refs.append(ref)
        _cache[key] = refs
    return _cache[key]


def _launch(dev, in_name, out_name, alias, aug=None):
    s = _setup(dev)
    aug = aug or s["aug"]
    in_dt, out_dt = DTYPES[in_name], DTYPES[out_name]
    rows, L = s["rows"], s["L"]
    B = len(rows)
    host = torch.full((B, L + 7), 0.77 if in_dt == torch.float32 else 25000, dtype=in_dt)      # in_pitch > L
    host[:, :L] = torch.from_numpy(s["xs"][in_name])
    for b, row in enumerate(rows):                       # whatever lies past a row's length is never read
        host[b, row[0]:L] = 0.55 if in_dt == torch.float32 else 17000
    wave = host.to(dev)
    lens = torch.tensor([r[0] for r in rows], dtype=torch.int32)
    params = torch.tensor([r[1:] for r in rows], dtype=torch.int32)
    if alias:
        assert in_dt == out_dt
        buf = wave
    else:
        buf = torch.full((B, L + 5), CANARY[out_dt], dtype=out_dt, device=dev)
    out, out_lens, stats = aug(wave[:, :L], lens, params, out_dtype=out_dt, out=buf)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), out_lens.cpu().numpy(), stats.cpu().numpy(), host.numpy()


def _check(dev, in_name, out_name, alias, aug=None):
    s = _setup(dev)
    refs = _reference(dev, in_name)
    res, out_lens, stats, host = _launch(dev, in_name, out_name, alias, aug)
    rows, L = s["rows"], s["L"]
    assert out_lens.tolist() == [r[0] for r in rows]
    if alias:
        assert np.array_equal(res[:, L:], host[:, L:]), "elements past L are untouched"
    else:
        assert (res[:, L:] == CANARY[DTYPES[out_name]]).all(), "canary past L"
    worst = 0.0
    for b, ((n, r, c, start, snr), ref) in enumerate(zip(rows, refs)):
        ex, ey, en = stats[b]
        rx, ry, rn = ref["stats"]
        assert abs(ex - rx) <= 1e-9 * rx and abs(en - rn) <= 1e-9 * rn, ("E_x / E_n", b, stats[b], ref["stats"])
        assert abs(ey - ry) <= 2.0 * np.linalg.norm(ref["e"]) * np.sqrt(ry) + 1e-9 * ry, ("E_y", b, ey, ry)
        assert (res[b, n:L] == 0).all(), ("zero fill", b)
        if r < 0 and c < 0:
            if in_name == out_name:
                assert np.array_equal(res[b, :n].view(np.uint8), host[b, :n].view(np.uint8)), ("identity copy", b)
                continue
        gs, gn = O.gains(ex, ey, en, r >= 0, c >= 0, snr)
        gs, gn = float(np.float32(gs)), float(np.float32(gn))
        want = gs * ref["y"] + gn * ref["v"]
        bound = gs * ref["e"] + 2.0 ** -22 * (np.abs(gs * ref["y"]) + np.abs(gn * ref["v"]))
        got = res[b, :n].astype(np.float64)
        if out_name == "pcm16":
            want, bound = np.clip(32768.0 * want, -32768.0, 32767.0), 0.5 + 32768.0 * bound
        ratio = np.abs(got - want) / np.maximum(bound, 1e-300)
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), ("output", b, rows[b], float(ratio.max()))
    print("wave_aug %s->%s alias=%s: worst |err| / bound = %.3f over %d rows" % (in_name, out_name, alias, worst, len(rows)))


@pytest.mark.parametrize("in_name,out_name,alias", [("f32", "f32", False), ("f32", "pcm16", False), ("pcm16", "f32", False),
                                                    ("pcm16", "pcm16", False), ("f32", "f32", True), ("pcm16", "pcm16", True)])
def test_parity_all_modes_in_one_launch(dev, in_name, out_name, alias):
    _check(dev, in_name, out_name, alias)


def test_parity_with_an_f32_noise_bank(dev):
    from lightning_asr_amd import ops
    s = _setup(dev)
    aug = ops.WaveAugmenter(s["rirs"], [n.astype(np.float32) / np.float32(32768.0) for n in s["noises"]], dev, noise_dtype=torch.float32)
    _check(dev, "f32", "f32", False, aug)


def test_fir_error_against_an_f32_emulation(dev):
    """the second FIR gate: per row, the kernel's largest error against the f64 oracle is at most 4 x that of an ascending-order
    numpy-f32 loop on the same row, floored at 2^-24 max A"""
    s = _setup(dev)
    refs = _reference(dev, "f32")
    _launch(dev, "f32", "f32", False)
    y_gpu = s["aug"].fir_rows(len(s["rows"]), s["L"]).cpu().numpy().astype(np.float64)
    img = s["aug"].rir_bank.cpu().numpy()
    worst = 0.0
    for b, ((n, r, c, start, snr), ref) in enumerate(zip(s["rows"], refs)):
        if r < 0:
            continue
        K, d, off = [int(v) for v in img[4 + 4 * r:7 + 4 * r]]
        h = img.view(np.float32)[off:off + K]
        emu, _ = O.fir(s["xs"]["f32"][b, :n], h, d, emulate_f32=True)
        err_emu = np.abs(emu - ref["y"]).max()
        err_gpu = np.abs(y_gpu[b, :n] - ref["y"]).max()
        yard = max(err_emu, 2.0 ** -24 * ref["A"].max())
        worst = max(worst, err_gpu / yard)
        assert err_gpu <= 4.0 * yard, (b, n, K, d, err_gpu, err_emu)
    print("wave_aug FIR: worst (kernel error) / max(f32 emulation error, 2^-24 max A) = %.3f" % worst)


def _small(dev):
    from lightning_asr_amd import ops
    if "small" not in _cache:
        rng = np.random.RandomState(3)
        _cache["small"] = ops.WaveAugmenter([make_rir(40, 3, 1), make_rir(9, 0, 2)],
                                            [np.zeros(50, dtype=np.int16), np.rint(rng.uniform(-0.5, 0.5, 300) * 32768).astype(np.int16)], dev)
    return _cache["small"]


def test_zero_speech_and_zero_noise_give_zero_gain(dev):
    aug = _small(dev)
    n = 500
    x = torch.from_numpy(np.random.RandomState(1).uniform(-0.5, 0.5, (4, n)).astype(np.float32))
    x[0] = 0
    x[1] = 0
    params = torch.tensor([[0, 1, 5, 1000], [-1, 1, 0, 1000], [0, 0, 7, 1000], [-1, 0, 49, 1000]], dtype=torch.int32)
    out, lens, stats = aug(x.to(dev), torch.full((4,), n, dtype=torch.int32), params)
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(stats).all()
    assert (out[:2] == 0).all() and (stats[:2, :2] == 0).all(), "silence in, silence out: both gains are zero"
    assert (stats[2:, 2] == 0).all()
    assert np.array_equal(out[3], x[3].numpy()), "zero noise adds nothing: g_s = 1, g_n = 0"
    assert abs(float((out[2].astype(np.float64) ** 2).sum()) / stats[2, 0] - 1.0) < 1e-5, "the reverberated row keeps the speech's power"
    assert lens.cpu().tolist() == [n] * 4


def test_pcm16_output_saturates(dev):
    aug = _small(dev)
    n = 400
    x = np.zeros((1, n), dtype=np.float32)
    x[0, ::2], x[0, 1::2] = 3.0, -3.0
    params = torch.tensor([[-1, 1, 0, 2000]], dtype=torch.int32)
    out, _, _ = aug(torch.from_numpy(x).to(dev), torch.tensor([n], dtype=torch.int32), params, out_dtype=torch.int16)
    out = out.cpu().numpy()[0]
    assert (out[::2] == 32767).all() and (out[1::2] == -32768).all()


@pytest.mark.parametrize("name", ["f32", "pcm16"])
def test_identity_rows_are_copied_with_their_lead_word(dev, name):
    aug = _small(dev)
    n, L = 300, 310
    rng = np.random.RandomState(4)
    if name == "f32":
        bits = rng.randint(0, 2 ** 32, (3, L), dtype=np.uint64).astype(np.uint32)        # any bit pattern, NaNs and denormals included
        host = torch.from_numpy(bits.view(np.float32).copy())
    else:
        host = torch.from_numpy(rng.randint(-32768, 32768, (3, L)).astype(np.int16))
    lens = torch.tensor([n | LEAD, n, 0], dtype=torch.int32, device=dev)
    params = torch.full((3, 4), -1, dtype=torch.int32, device=dev)
    out, out_lens, _ = aug(host.to(dev), lens, params)
    got = out.cpu()
    assert out_lens.cpu().tolist() == [n | LEAD, n, 0]
    view = (lambda t: t.numpy().view(np.uint32)) if name == "f32" else (lambda t: t.numpy())
    assert np.array_equal(view(got[0, :n + 1]), view(host[0, :n + 1])) and (view(got[0, n + 1:]) == 0).all()
    assert np.array_equal(view(got[1, :n]), view(host[1, :n])) and (view(got[1, n:]) == 0).all()
    assert (view(got[2]) == 0).all()
    with pytest.raises(ValueError, match="lead-in"):
        aug(host.to(dev), lens.cpu(), torch.tensor([[0, -1, 0, 0]] * 3, dtype=torch.int32))


def test_bad_ids_and_a_damaged_bank_give_zero_rows(dev):
    aug = _small(dev)
    n = 2100
    x = torch.from_numpy(np.random.RandomState(2).uniform(-0.5, 0.5, (8, n)).astype(np.float32)).to(dev)
    lens = torch.full((8,), n, dtype=torch.int32, device=dev)
    params = torch.tensor([[2, -1, 0, 0], [300, -1, 0, 0], [-1, 2, 0, 0], [-1, 1, 300, 0], [-1, 1, -1, 0], [0, 7, 0, 0],
                           [1, 1, 299, 1500], [-1, -1, 0, 0]], dtype=torch.int32, device=dev)
    out, out_lens, stats = aug(x, lens, params)
    assert out_lens.cpu().tolist() == [0] * 6 + [n, n]
    assert (out[:6] == 0).all() and (stats[:6] == 0).all()
    assert (out[6] != 0).any() and torch.equal(out[7], x[7])
    good = aug.rir_bank.clone()
    try:
        for word, value in ((0, 7), (1, 1000), (2, 1 << 22), (4, 9000), (5, 40), (6, 1 << 21), (6, 1030), (6, 8)):
            aug.rir_bank = good.clone()
            aug.rir_bank[word] = value                       # magic, count, image size, K, d, offset (far, unaligned, inside the header)
            out, out_lens, _ = aug(x, lens, torch.tensor([[0, -1, 0, 0]] * 8, dtype=torch.int32, device=dev))
            assert out_lens.cpu().tolist() == [0] * 8 and (out == 0).all(), (word, value)
        aug.rir_bank = good[:good.numel() - 4].clone()       # an image cut short: its entries end past the words handed in
        out, out_lens, _ = aug(x, lens, torch.tensor([[1, -1, 0, 0]] * 8, dtype=torch.int32, device=dev))
        assert out_lens.cpu().tolist() == [0] * 8 and (out == 0).all()
    finally:
        aug.rir_bank = good


def test_two_runs_are_bitwise_equal_and_a_graph_replays_the_eager_result(dev):
    aug = _small(dev)
    B, n = 6, 5000
    x = torch.from_numpy(np.random.RandomState(6).uniform(-0.5, 0.5, (B, n)).astype(np.float32)).to(dev)
    lens = torch.tensor([n, n - 1, 2049, 2048, 1, n], dtype=torch.int32, device=dev)
    params = torch.tensor([[0, 1, 5, 1000], [1, -1, 0, 0], [-1, 1, 299, 700], [0, 1, 0, 1999], [1, 1, 3, 500], [-1, -1, 0, 0]],
                          dtype=torch.int32, device=dev)
    a = [t.clone() for t in aug(x, lens, params)]
    b = [t.clone() for t in aug(x, lens, params)]
    for u, v in zip(a, b):
        assert np.array_equal(u.cpu().numpy().view(np.uint8), v.cpu().numpy().view(np.uint8))
    out, out_lens, stats = torch.zeros_like(a[0]), torch.zeros_like(a[1]), torch.zeros_like(a[2])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        aug(x, lens, params, out=out, out_lens=out_lens, stats=stats)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    for u, v in zip(a, (out, out_lens, stats)):
        assert np.array_equal(u.cpu().numpy().view(np.uint8), v.cpu().numpy().view(np.uint8))
