"""Host tier of the noise and reverberation augmentation (no GPU): the f64 oracle against scipy, the RIR bank image against the
oracle's geometry, every hostile input refused, conf parsing, the draws of the training routes and the metadata block."""
import json
import os
import random
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import wave_aug_oracle as O  # noqa: E402


def decaying(K, seed, tau=None):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(K) * np.exp(-np.arange(K) / (tau or K / 7.0))).astype(np.float32)


def entries(img, n):
    return [tuple(int(v) for v in img[4 + 4 * i:7 + 4 * i]) for i in range(n)]


def test_oracle_fir_agrees_with_scipy_fftconvolve():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.RandomState(0)
    for n, K, d in ((1, 1, 0), (50, 7, 0), (50, 7, 6), (333, 120, 40), (2000, 901, 900), (64, 300, 150)):
        x, h = rng.uniform(-1, 1, n), decaying(K, K).astype(np.float64)
        y, a = O.fir(x, h, d)
        full = signal.fftconvolve(x, h)                       # full[m] = sum_k h[k] x[m - k]; y[j] = full[j + d]
        want = np.concatenate([full, np.zeros(n + K)])[d:d + n]
        assert np.abs(y - want).max() < 1e-12 and (a >= np.abs(y) - 1e-15).all()
    x = rng.uniform(-1, 1, 40)
    assert np.array_equal(O.noise_row(np.arange(7.0), 6, 10), np.array([6, 0, 1, 2, 3, 4, 5, 6, 0, 1.0]))
    r = O.augment(x, None, 0, rng.uniform(-1, 1, 9), 8, 1000)
    assert abs(10 * np.log10(r["stats"][0] / (r["gains"][1] ** 2 * r["stats"][2])) - 10.0) < 1e-9, "the mix has the asked SNR"
    r = O.augment(x, decaying(12, 1).astype(np.float64), 3)
    assert abs((r["out"] ** 2).sum() / r["stats"][0] - 1.0) < 1e-12, "reverberation keeps the speech's power"


def test_bank_image_matches_the_oracle():
    from lightning_asr_amd import ops
    rirs = [decaying(300, 1), decaying(4000, 2, tau=150.0), decaying(20000, 3, tau=4000.0)]        # the last is longer than the cap
    first = decaying(64, 4)
    first[0] = 5.0                                            # peak at index 0
    last = decaying(64, 5) * 0.1
    last[63] = 3.0                                            # peak at the last kept tap
    tie = np.array([0.2, -0.7, 0.7, 0.1], dtype=np.float32)   # the FIRST of two equal peaks
    pcm = (decaying(100, 6) * 8000).astype(np.int16)          # int16 RIRs are scaled by 1 / 32768
    rirs += [first, last, tie, pcm]
    img = ops.rir_bank_image(rirs)
    words = img.numpy()
    assert words[0] == 0x52495231 and words[1] == len(rirs) and words[2] == words.size and words[3] == 0
    expect_off = 4 + 4 * 256
    got = entries(words, len(rirs))
    for i, (h, (K, d, off)) in enumerate(zip(rirs, got)):
        h = h.astype(np.float32) / 32768.0 if h.dtype == np.int16 else h
        assert (d, K) == O.rir_geometry(h), i
        assert off == expect_off and off % 4 == 0
        taps = words.view(np.float32)[off:off + K]
        assert np.array_equal(taps, h[:K]), "taps are stored unscaled"
        nxt = got[i + 1][2] if i + 1 < len(rirs) else words.size         # zero taps up to the kernel's step: a few words at most
        assert 0 <= nxt - off - K < 16 and (nxt - off) % 4 == 0 and (words[off + K:nxt] == 0).all()
        expect_off = nxt
    assert expect_off == words.size
    assert got[2][0] == 8192 and got[3][1] == 0 and got[4][:2] == (64, 63) and got[5][:2] == (4, 1)
    assert got[1][0] < 4000, "a tail below 1e-6 of the energy is dropped"
    assert ops.rir_bank_image([]).numel() == 4 + 4 * 256
    assert ops.wave_augment_tile() % 64 == 0 and ops.wave_augment_chunk() % 4 == 0


def test_hostile_rirs_are_refused():
    from lightning_asr_amd import _lib, ops
    ok = decaying(32, 1)
    late = np.zeros(9000, dtype=np.float32)
    late[8192] = 1.0
    cases = [([ok, np.zeros(0, dtype=np.float32)], "RIR 1"), ([np.zeros(5, dtype=np.float32)], "RIR 0"),
             ([ok, ok, np.array([1, np.nan], dtype=np.float32)], "RIR 2"), ([np.array([np.inf], dtype=np.float32), ok], "RIR 0"),
             ([np.ones((1 << 20) + 1, dtype=np.float32)], "RIR 0"), ([late], "RIR 0"), ([ok] * 257, "256")]
    big = np.full(8192, 0.5, dtype=np.float32)
    big[0] = 1.0
    cases.append(([big] * 256, "RIR 255"))
    for rirs, names in cases:
        with pytest.raises(_lib.LasrError, match=names):
            ops.rir_bank_image(rirs)
    for bad in (np.zeros((2, 2), dtype=np.float32), np.zeros(4, dtype=np.float64), [1.0, 2.0]):
        with pytest.raises(ValueError):
            ops.rir_bank_image([bad])
    lib = _lib.load()
    assert lib.lasr_wave_augment_workspace_bytes(70000, 10) == 0 and lib.lasr_wave_augment_workspace_bytes(1, 1 << 31) == 0
    assert lib.lasr_wave_augment_workspace_bytes(2, 1) >= 2 * ops.wave_augment_tile() * 4


def test_conf_parsing():
    from lightning_asr_amd.data_module import WaveAugConfig
    c = WaveAugConfig()
    assert not c.on and (c.noise_prob, c.rir_prob, c.noise_snr_db, c.noise_max_seconds) == (0.5, 0.3, (5.0, 20.0), 600.0)
    c = WaveAugConfig("n.json", 1, [10, 10], 5, "r.json", 0)
    assert c.on and c.noise_manifest == "n.json" and c.rir_manifest == "r.json" and c.noise_snr_db == (10.0, 10.0)
    for kw, key in ((dict(noise_prob=1.5), "noise_prob"), (dict(noise_prob=-0.1), "noise_prob"), (dict(rir_prob=float("nan")), "rir_prob"),
                    (dict(rir_prob="0.3"), "rir_prob"), (dict(noise_snr_db=[20, 5]), "noise_snr_db"), (dict(noise_snr_db=7), "noise_snr_db"),
                    (dict(noise_snr_db=[1, 2, 3]), "noise_snr_db"), (dict(noise_max_seconds=0), "noise_max_seconds"),
                    (dict(noise_max_seconds=-3), "noise_max_seconds"), (dict(noise_max_seconds=float("inf")), "noise_max_seconds")):
        with pytest.raises(ValueError, match=key):
            WaveAugConfig(**kw)
    import yaml
    data = yaml.safe_load(open(os.path.join(ROOT, "conf", "conf.yaml")))["data"]
    c = WaveAugConfig(data["noise_manifest"], data["noise_prob"], data["noise_snr_db"], data["noise_max_seconds"], data["rir_manifest"], data["rir_prob"])
    assert not c.on and c.noise_prob == 0.5 and c.rir_prob == 0.3 and c.noise_snr_db == (5.0, 20.0) and c.noise_max_seconds == 600.0


def _write_wav(path, rate, pcm):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


def test_manifest_loading_and_its_budget(tmp_path):
    from lightning_asr_amd.data_module import AudioParser, load_aug_manifest
    ap = AudioParser.__new__(AudioParser)
    ap.sr = 16000
    rng = np.random.RandomState(2)
    man = tmp_path / "noise.json"
    clips = [rng.randint(-9000, 9000, size=n).astype(np.int16) for n in (16000, 8000, 12000)]
    with open(man, "w") as f:
        for i, c in enumerate(clips):
            _write_wav(tmp_path / ("n%d.wav" % i), 16000, c)
            f.write(json.dumps({"audio_filepath": str(tmp_path / ("n%d.wav" % i))}) + "\n")
    got = load_aug_manifest(str(man), "noise_manifest", ap, 600)
    assert [g.size for g in got] == [16000, 8000, 12000] and np.array_equal(got[1], clips[1].astype(np.float32) / 32768.0)
    got = load_aug_manifest(str(man), "noise_manifest", ap, 1.25)          # the budget: manifest order, the last file cut at it
    assert [g.size for g in got] == [16000, 4000]
    empty = tmp_path / "empty.json"
    empty.write_text("\n")
    with pytest.raises(ValueError, match="rir_manifest"):
        load_aug_manifest(str(empty), "rir_manifest", ap)


def test_draw_sequence():
    from lightning_asr_amd.data_module import WaveAug
    rirs, noises = [np.ones(3, dtype=np.float32)] * 5, [np.ones(n, dtype=np.int16) for n in (10, 200, 3000)]
    wa = WaveAug(rirs, noises, rir_prob=0.4, noise_prob=0.6, noise_snr_db=(5, 20))
    a, b = random.Random(11), random.Random(11)
    for _ in range(200):
        got = wa.draw(a)
        rir = nid = -1
        start = snr = 0
        if b.random() < 0.4:
            rir = b.randrange(5)
        if b.random() < 0.6:
            nid = b.randrange(3)
            start = b.randrange([10, 200, 3000][nid])
            snr = int(round(100 * b.uniform(5, 20)))
        assert got == (rir, nid, start, snr)
    assert a.random() == b.random()
    # a kind that is off draws nothing; with both off nothing is drawn at all
    a, b = random.Random(5), random.Random(5)
    only_noise = WaveAug([], noises, rir_prob=1.0, noise_prob=1.0, noise_snr_db=(7, 7))
    r = only_noise.draw(a)
    b.random(); nid = b.randrange(3); start = b.randrange([10, 200, 3000][nid]); b.uniform(7, 7)      # noqa: E702
    assert r == (-1, nid, start, 700) and a.random() == b.random()
    a, b = random.Random(6), random.Random(6)
    assert WaveAug(rirs, [], rir_prob=0.0).draw(a) == (-1, -1, 0, 0)
    b.random()
    assert a.random() == b.random()
    a, b = random.Random(7), random.Random(7)
    assert WaveAug([], []).draw(a) == (-1, -1, 0, 0) and a.random() == b.random()


def test_batch_producer_draws_and_metadata(tmp_path):
    """the host half of the native route: per clip speed factor, parameter word, rectangle; the words behind the speed tail; no
    lead-in samples; with the keys off the metadata block is byte for byte today's"""
    from lightning_asr_amd import ingest
    from lightning_asr_amd.data_module import AudioParser, MyAudioDataset, WaveAug, parse_speed_factors
    rng = np.random.RandomState(1)
    man = tmp_path / "m.json"
    ns = [8000 + 1000 * i for i in range(3)]
    with open(man, "w") as f:
        for i, n in enumerate(ns):
            p = tmp_path / ("c%d.wav" % i)
            _write_wav(p, 16000, rng.randint(-1000, 1000, size=n).astype(np.int16))
            f.write(json.dumps({"audio_filepath": str(p), "duration": n / 16000.0, "text": "ab"}) + "\n")
    ds = MyAudioDataset([str(man)], list("abcdefg"), mask=True)
    rirs, noises = [np.ones(3, dtype=np.float32)] * 4, [np.ones(n, dtype=np.int16) for n in (50, 5000)]

    def parser(seed, speed=False, aug=True):
        ap = AudioParser.__new__(AudioParser)
        ap.rand = random.Random(seed)
        ap.speed_factors = parse_speed_factors([0.9, 1.0, 1.1]) if speed else []
        ap.wave_aug = WaveAug(rirs, noises, rir_prob=0.5, noise_prob=0.7) if aug else None
        return ap

    ring = ingest.PinnedRing(1, 3 * 12000, 16, pin=False)
    for speed in (False, True):
        prod = ingest.BatchProducer(ds, [[0, 1, 2]], ring, mask=True, audio_parser=parser(3, speed), n_threads=1, crop=False, speed=speed,
                                    wave_aug=True)
        hb = prod.make([0, 1, 2], 0)
        twin = parser(3, speed)
        ks, n_out, words, rects = [], [], [], []
        for n in ns:
            if speed:
                ks.append(twin.draw_speed())
                n = twin.speed_out_len(n, ks[-1])
            n_out.append(n)
            words.append(twin.draw_wave_aug())
            rects.append(list(twin.draw_spec_augment(1 + (n + 64) // 160)))
        assert hb.wave_aug == words and hb.lens.tolist() == n_out and hb.aug.tolist() == rects and hb.speed == (ks if speed else None)
        base = ingest.Layout(3, hb.S, True, speed).words
        lay = ingest.Layout(3, hb.S, True, speed, True)
        assert hb.layout.words == lay.words == base + 12 and lay.params == base
        assert hb.meta[base:base + 12].view(3, 4).tolist() == [list(w) for w in words]
        assert lay.views(hb.meta).params.tolist() == [list(w) for w in words]
    # the crop on: never a lead-in sample
    np.random.seed(0)
    hb2 = ingest.BatchProducer(ds, [[0, 1, 2]], ring, mask=True, audio_parser=parser(3), n_threads=1, crop=True, wave_aug=True).make([0, 1, 2], 0)
    assert all(0 < v < n for v, n in zip(hb2.lens.tolist(), ns))
    # keys off (no WaveAug on the parser, or wave_aug=False): the block of before, byte for byte, and the same draws
    blocks = []
    for kw, aug in ((dict(), False), (dict(wave_aug=True), False), (dict(wave_aug=False), True)):
        hb3 = ingest.BatchProducer(ds, [[0, 1, 2]], ring, mask=True, audio_parser=parser(9, aug=aug), n_threads=1, crop=False, **kw).make([0, 1, 2], 0)
        assert hb3.wave_aug is None and hb3.speed is None and hb3.layout.words == ingest.Layout(3, hb3.S, True).words
        blocks.append(hb3.meta[:hb3.layout.words].numpy().tobytes())
    twin = parser(9, aug=False)
    rects = [list(twin.draw_spec_augment(1 + (n + 64) // 160)) for n in ns]
    lay = ingest.Layout(3, 2, True)
    want = np.zeros(lay.words, dtype=np.int32)
    want[lay.lens:lay.lens + 3], want[lay.sizes:lay.sizes + 3] = ns, [2, 2, 2]
    want[lay.aug:lay.aug + 12] = np.asarray(rects, dtype=np.int32).reshape(-1)
    want[lay.targets:lay.targets + 12].view(np.int64)[:] = [0, 1] * 3
    assert blocks[0] == blocks[1] == blocks[2] == want.tobytes()

    def offsets(*a):
        lay = ingest.Layout(*a)
        return lay.lens, lay.sizes, lay.aug, lay.targets, lay.words, lay.raw_lens, lay.conv, lay.params
    assert offsets(5, 7, True)[:5] == (0, 5, 10, 30, 100) and offsets(5, 7, False, True)[:5] == (0, 5, 10, 10, 90)
    assert offsets(5, 7, False, True)[5:] == (80, 85, 90) and offsets(5, 7, True, False, True)[4:] == (120, 100, 100, 100)
    assert offsets(5, 7, True, True, True) == (0, 5, 10, 30, 130, 100, 105, 110)
