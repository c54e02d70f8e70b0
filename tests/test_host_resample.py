"""CPU tier of the resampler: the bank the library builds against the numpy f64 oracle (tests/helpers/resample_oracle.py), the
output length, refusals, the oracle itself against scipy's polyphase filter, and the host plumbing (speed-factor parsing,
``load_wav_rate``).  No GPU."""
import ctypes
import math
import os
import sys
import wave
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_oracle as O  # noqa: E402

from lightning_asr_amd import _lib  # noqa: E402

CONVERSIONS = [(44100, 16000), (22050, 16000), (48000, 16000), (8000, 16000), (9, 10), (11, 10)]
E_ARG = -1


def _rates(convs):
    n = max(len(convs), 1)
    return (ctypes.c_int32 * n)(*[c[0] for c in convs]), (ctypes.c_int32 * n)(*[c[1] for c in convs])


def bank_image(convs, lpw=6, rolloff=0.99):
    lib = _lib.load()
    a, b = _rates(convs)
    nbytes = lib.lasr_resample_bank_bytes(a, b, len(convs), lpw, rolloff)
    assert nbytes > 0, lib.lasr_last_error()
    img = np.full(nbytes // 4 + 4, 0x5A5A5A5A, dtype=np.int32)          # 4 guard words behind the image
    assert lib.lasr_resample_bank_write(a, b, len(convs), lpw, rolloff, img.ctypes.data, nbytes) == 0, lib.lasr_last_error()
    assert (img[-4:] == 0x5A5A5A5A).all()
    return img[:-4]


def bank_taps(img, i):
    """(up, taps) f32 taps of conversion i, from the image's [tap][phase] layout"""
    up, down, width, taps, offset = [int(v) for v in img[16 + 8 * i:21 + 8 * i]]
    return img.view(np.float32)[offset:offset + up * taps].reshape(taps, up).T, (up, down, width, taps)


def test_bank_matches_the_oracle_taps():
    img = bank_image(CONVERSIONS)
    assert int(img[1]) == len(CONVERSIONS)
    for i, (a, b) in enumerate(CONVERSIONS):
        h32, geo = bank_taps(img, i)
        assert geo == O.geometry(a, b), (a, b, geo)
        h = O.taps(a, b)
        err = np.abs(h32.astype(np.float64) - h)
        bound = 2.0 ** -24 * np.abs(h) + 1e-15      # one rounding to f32 + f64 libm noise near the filter's zeros
        assert (err <= bound).all(), (a, b, float((err - bound).max()))
    # one conversion alone is the same bank entry
    alone, _ = bank_taps(bank_image([CONVERSIONS[0]]), 0)
    assert np.array_equal(alone, bank_taps(img, 0)[0])


def test_geometry_known_answers():
    assert O.geometry(44100, 16000) == (160, 441, 17, 475)
    assert O.geometry(48000, 16000) == (1, 3, 19, 41)
    assert O.geometry(8000, 16000) == (2, 1, 7, 15)
    assert O.geometry(9, 10) == (10, 9, 7, 23)
    assert O.geometry(11, 10) == (10, 11, 7, 25)
    for a, b in CONVERSIONS:                           # per-phase DC gain
        s = O.taps(a, b).sum(axis=1)
        assert s.min() > 0.9999 and s.max() < 1.0010, (a, b, s.min(), s.max())
    # a sine at 0.01 sr_in comes back to better than 1e-3 away from the edges
    n = np.arange(4410)
    y, _ = O.resample(np.sin(2 * np.pi * 0.01 * n), 44100, 16000)
    t = np.arange(y.size) * 441 / 160
    assert np.abs(y - np.sin(2 * np.pi * 0.01 * t))[40:-40].max() < 1e-3


def test_out_len_is_ceil():
    lib = _lib.load()
    for a, b in CONVERSIONS:
        up, down, _, _ = O.geometry(a, b)
        for n in (0, 1, 2, down - 1, down, down + 1, 159999):
            if n < 0:
                continue
            want = int(math.ceil(Fraction(n * up, down)))
            assert lib.lasr_resample_out_len(n, up, down) == want == O.out_len(n, up, down), (a, b, n)
    for bad in ((-1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1025, 1), (1, 1, 1025), (2 ** 63 - 1, 1024, 1)):
        assert lib.lasr_resample_out_len(*bad) == -1, bad


def test_hostile_arguments_are_refused():
    lib = _lib.load()
    ok = [(8000, 16000)]

    def refused(convs, n=None, lpw=6, rolloff=0.99):
        a, b = _rates(convs)
        n = len(convs) if n is None else n
        buf = np.zeros(64, np.int32)
        assert lib.lasr_resample_bank_bytes(a, b, n, lpw, rolloff) == 0, (convs, n, lpw, rolloff)
        assert lib.lasr_resample_bank_write(a, b, n, lpw, rolloff, buf.ctypes.data, buf.nbytes) == E_ARG, (convs, n, lpw, rolloff)
        assert lib.lasr_last_error()

    for convs in ([(0, 16000)], [(16000, 0)], [(-8000, 16000)], [(16000, -1)], [(1025, 1)], [(1, 1025)], [(16000, 16001)],
                  [(44101, 16000)], [(1023, 1024)], ok * 9):
        refused(convs)
    refused(ok, n=0)
    refused(ok, n=-3)
    for r in (0.0, -0.1, 1.0001, float("nan"), float("inf"), 5e-324, 1e-9):
        refused(ok, rolloff=r)
    for lpw in (0, -1, 65, 2 ** 31 - 1):
        refused(ok, lpw=lpw)
    refused([(1024, 1)], lpw=64, rolloff=0.01)         # up * taps above 2^20
    assert lib.lasr_resample_bank_bytes(None, None, 1, 6, 0.99) == 0
    # a destination one byte short, and none at all
    a, b = _rates(ok)
    nbytes = lib.lasr_resample_bank_bytes(a, b, 1, 6, 0.99)
    buf = np.zeros(nbytes // 4, np.int32)
    assert lib.lasr_resample_bank_write(a, b, 1, 6, 0.99, buf.ctypes.data, nbytes - 1) == E_ARG
    assert lib.lasr_resample_bank_write(a, b, 1, 6, 0.99, None, nbytes) == E_ARG
    assert not buf.any()
    assert lib.lasr_resample(None, None, 0, 0, None, None, None, 0, 0, 0, None, 1, None) == E_ARG     # nothing launched
    assert lib.lasr_resample_tile(0, 1, 6, 0.99) == -1 and lib.lasr_resample_tile(4, 2, 6, 0.99) == -1


def test_oracle_agrees_with_scipy_upfirdn():
    """the oracle is a polyphase FIR with prototype g[m] = h[m % up][m // up] delayed by width * up output samples: where that
    delay is a whole number of OUTPUT samples after decimation (48000 -> 16000, 8000 -> 16000) scipy computes the same sums"""
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.RandomState(5)
    for a, b in ((48000, 16000), (8000, 16000)):
        up, down, width, taps = O.geometry(a, b)
        h = O.taps(a, b)
        # out[j] = sum_k h[j % up][k] x[(j // up) * down + k - width]; upfirdn: y[n] = sum_i g[n * down - i * up] x[i]
        # with i = q * down + k - width, n = j: g[j * down - (q * down + k - width) * up], j = q * up + p
        #   = g[p * down + (width - k) * up]  ->  g[m] with m = p * down + (width - k) * up; shift m by an offset to make it >= 0
        lo = min(p * down + (width - k) * up for p in range(up) for k in range(taps))
        g = np.zeros(max(p * down + (width - k) * up for p in range(up) for k in range(taps)) - lo + 1)
        for p in range(up):
            for k in range(taps):
                g[p * down + (width - k) * up - lo] = h[p, k]
        assert (-lo) % down == 0                        # the delay is a whole number of output samples
        x = rng.uniform(-0.9, 0.9, 1000)
        full = sig.upfirdn(g, x, up, down)
        y, _ = O.resample(x, a, b)
        d = (-lo) // down
        assert np.abs(full[d:d + y.size] - y).max() < 1e-12


def test_speed_factor_parsing():
    from lightning_asr_amd.data_module import parse_speed_factors
    assert parse_speed_factors(None) == [] and parse_speed_factors([]) == []
    assert parse_speed_factors([0.9, 1.0, 1.1]) == [Fraction(9, 10), Fraction(1), Fraction(11, 10)]
    assert parse_speed_factors(["0.95", 1, 2, 0.5, "3/4"]) == [Fraction(19, 20), Fraction(1), Fraction(2), Fraction(1, 2), Fraction(3, 4)]
    for bad in ([0.49], [2.01], [0], [-1.0], ["fast"], [float("nan")], [0.9001], [1 / 3], 0.9, "0.9", [None], [[0.9]],
                [1.0 + i / 100 for i in range(9)]):
        with pytest.raises(ValueError):
            parse_speed_factors(bad)


def _write_wav(path, rate, pcm, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


def test_load_wav_rate_returns_the_header_rate(tmp_path):
    from lightning_asr_amd.data_module import load_wav, load_wav_rate
    rng = np.random.RandomState(1)
    for rate in (8000, 16000, 22050, 44100, 48000):
        pcm = rng.randint(-30000, 30000, size=321).astype(np.int16)
        p = tmp_path / ("r%d.wav" % rate)
        _write_wav(p, rate, pcm)
        y, sr = load_wav_rate(str(p))
        assert sr == rate and y.shape == (1, 321)
        assert np.array_equal(y.numpy()[0], pcm.astype(np.float32) / 32768.0)
        assert np.array_equal(load_wav(str(p)).numpy(), y.numpy())           # load_wav: the same wave, rate dropped as before
        with open(p, "rb") as f:                                              # file objects too
            assert load_wav_rate(f)[1] == rate
    st = tmp_path / "stereo.wav"
    _write_wav(st, 44100, rng.randint(-100, 100, size=2 * 50).astype(np.int16), channels=2)
    y, sr = load_wav_rate(str(st))
    assert sr == 44100 and y.shape == (1, 50)


def test_batch_producer_draws_speed_factors(tmp_path):
    """the host half of the native route: raw PCM in the ring slot, the resampled lengths in `lens`, the raw lengths and the
    conversions behind the targets, rectangles drawn for the resampled lengths, no lead-in samples even with the crop on"""
    import json
    import random
    from lightning_asr_amd import ingest
    from lightning_asr_amd.data_module import AudioParser, MyAudioDataset, parse_speed_factors
    rng = np.random.RandomState(1)
    man = tmp_path / "m.json"
    ns = [8000 + 1000 * i for i in range(3)]
    with open(man, "w") as f:
        for i, n in enumerate(ns):
            p = tmp_path / ("c%d.wav" % i)
            _write_wav(p, 16000, rng.randint(-1000, 1000, size=n).astype(np.int16))
            f.write(json.dumps({"audio_filepath": str(p), "duration": n / 16000.0, "text": "ab"}) + "\n")
    ds = MyAudioDataset([str(man)], list("abcdefg"), mask=True)

    def parser(seed):
        ap = AudioParser.__new__(AudioParser)
        ap.rand = random.Random(seed)
        ap.speed_factors = parse_speed_factors([0.9, 1.0, 1.1])
        return ap

    ring = ingest.PinnedRing(1, 3 * 12000, 16, pin=False)
    prod = ingest.BatchProducer(ds, [[0, 1, 2]], ring, mask=True, audio_parser=parser(3), n_threads=1, crop=False, speed=True)
    hb = prod.make([0, 1, 2], 0)
    twin = parser(3)
    ks, n_out, rects = [], [], []
    for n in ns:
        ks.append(twin.draw_speed())
        n_out.append(twin.speed_out_len(n, ks[-1]))
        rects.append(list(twin.draw_spec_augment(1 + (n_out[-1] + 64) // 160)))
    assert hb.speed == ks and hb.lens.tolist() == n_out and hb.aug.tolist() == rects
    assert n_out == [int(math.ceil(n / Fraction(str([0.9, 1.0, 1.1][k])))) for n, k in zip(ns, ks)]
    assert abs(hb.seconds - sum(n_out) / 16000.0) < 1e-9 and hb.ld == 10000
    lay = ingest.Layout(3, hb.S, True, True)
    assert lay.words == hb.layout.words == ingest.Layout(3, hb.S, True).words + 6
    o_raw = lay.targets + 2 * 3 * hb.S
    assert o_raw == lay.raw_lens and o_raw + 3 == lay.conv
    assert hb.meta[o_raw:o_raw + 3].tolist() == ns and hb.meta[o_raw + 3:o_raw + 6].tolist() == ks
    # the crop on: slices of the files, but never a lead-in sample (the flag would be a caller error on a resampled row)
    np.random.seed(0)
    prod2 = ingest.BatchProducer(ds, [[0, 1, 2]], ring, mask=True, audio_parser=parser(3), n_threads=1, crop=True, speed=True)
    hb2 = prod2.make([0, 1, 2], 0)
    raw = hb2.meta[o_raw:o_raw + 3].tolist()
    assert all(0 < r < n for r, n in zip(raw, ns)) and all(v < (1 << 30) for v in hb2.lens.tolist())
    # off: the batch of before, and no speed record
    prod3 = ingest.BatchProducer(ds, [[0, 1, 2]], ring, mask=True, audio_parser=parser(3), n_threads=1, crop=False)
    hb3 = prod3.make([0, 1, 2], 0)
    assert hb3.speed is None and hb3.lens.tolist() == ns and hb3.layout.words == ingest.Layout(3, hb3.S, True).words
