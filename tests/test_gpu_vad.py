"""GPU tier of the voice-activity segmenter (csrc/segment.hip): ``ops.vad_segments`` against the numpy oracle of
tests/helpers/vad_oracle.py with ``torch.equal`` on the segments, their count, the noise floor and every frame level - the
arithmetic is integer, so there is no tolerance - and ``ops.gather_segments`` against slices.  Small parameters (min_silence 3,
min_speech 2, pad 1, max_frames 8) make every pass do work at a handful of frames; the row lengths sit around the frames one
workgroup takes per sweep (``ops.vad_sweep``)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vad_cases as K  # noqa: E402
import vad_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


def _frame_levels(amps: np.ndarray, n_samples: int) -> np.ndarray:
    """levels of the first n_samples of amplitude_wave(amps): whole frames have E = 160 a^2, the last one what is left of it"""
    F = -(-n_samples // 160)
    count = np.full(F, 160, dtype=np.int64)
    if F:
        count[-1] = n_samples - 160 * (F - 1)
    return O.levels_of_energy(count * amps[:F].astype(np.int64) ** 2)


def _assert_rows(res, want_levels, n_samples, P, Fp):
    """res: VadSegments of B rows; want_levels[b]: the oracle's levels of row b"""
    segs, n_segs, floor, levels = res.segs.cpu(), res.n_segs.cpu(), res.floor.cpu(), res.levels.cpu()
    for b, lev in enumerate(want_levels):
        want, want_floor = O.segment_levels(lev, n_samples[b], P)
        pad = np.zeros(Fp, dtype=np.int16)
        pad[:lev.size] = lev
        assert torch.equal(levels[b], torch.from_numpy(pad)), "levels of row %d" % b
        assert int(floor[b]) == want_floor, "floor of row %d" % b
        assert int(n_segs[b]) == want.shape[0], "row %d: %d segments, oracle %d" % (b, int(n_segs[b]), want.shape[0])
        assert torch.equal(segs[b, :want.shape[0]], torch.from_numpy(want)), "segments of row %d" % b


@pytest.mark.parametrize("case", K.hand_cases(), ids=lambda c: c["name"])
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["pcm16", "f32"])
def test_hand_cases(dev, case, dtype):
    from lightning_asr_amd import ops
    pcm = torch.from_numpy(case["wave"].copy())
    wave = (pcm if dtype == torch.int16 else pcm.float() / 32768.0).to(dev)
    res = ops.vad_segments(wave, max_segments=16, return_levels=True, **case["kwargs"])
    n = int(res.n_segs)
    assert [tuple(s) for s in res.segs[:n].cpu().tolist()] == case["want"]
    want, want_floor, lev = O.segment(case["wave"], O.params(**case["kwargs"]))
    assert torch.equal(res.segs[:n].cpu(), torch.from_numpy(want)) and int(res.floor) == want_floor
    assert torch.equal(res.levels.cpu(), torch.from_numpy(lev.astype(np.int16)))


def test_six_second_recording_with_the_default_parameters(dev):
    from lightning_asr_amd import ops
    pcm = O.recording_6s()
    want, want_floor, lev = O.segment(pcm, O.params())
    for wave in (torch.from_numpy(pcm).to(dev), (torch.from_numpy(pcm).float() / 32768.0).to(dev)):
        res = ops.vad_segments(wave, return_levels=True)
        assert int(res.n_segs) == 2 and torch.equal(res.segs[:2].cpu(), torch.from_numpy(want))
        assert int(res.floor) == want_floor and torch.equal(res.levels.cpu(), torch.from_numpy(lev.astype(np.int16)))
    assert [(s / 16000.0, e / 16000.0) for s, e in want.tolist()] == O.RECORDING_6S_SEGMENTS


def test_f32_samples_round_half_to_even_and_saturate(dev):
    from lightning_asr_amd import ops
    x = np.zeros(320, dtype=np.float32)
    x[:8] = [0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, 1.0, -1.0, 2.0, -3.0]
    x[160:164] = [3.5 / 32768, -2.5 / 32768, 1e-9, -1e30]
    res = ops.vad_segments(torch.from_numpy(x).to(dev), return_levels=True)
    assert torch.equal(res.levels.cpu(), torch.from_numpy(O.levels(x).astype(np.int16)))


@pytest.mark.parametrize("which", ["sweep-1", "sweep", "sweep+1", "3*sweep+1"])
def test_row_lengths_around_a_sweep(dev, which):
    from lightning_asr_amd import ops
    S = ops.vad_sweep()
    F = {"sweep-1": S - 1, "sweep": S, "sweep+1": S + 1, "3*sweep+1": 3 * S + 1}[which]
    rng = np.random.RandomState(F)
    amps = K.random_amps(rng, F)
    amps[S - 3:S + 3] = K.H                                                  # a run across the first sweep border
    n = 160 * F - 77
    wave = torch.from_numpy(amps).to(dev).repeat_interleave(160)[:n].contiguous()
    res = ops.vad_segments(wave.unsqueeze(0), max_segments=F, return_levels=True, **K.SMALL)
    _assert_rows(res, [_frame_levels(amps, n)], [n], O.params(**K.SMALL), F)
    assert int(res.n_segs[0]) > 100


def test_two_hundred_random_level_patterns_in_one_batch(dev):
    from lightning_asr_amd import ops
    rng = np.random.RandomState(2024)
    B, Fmax = 200, 3000
    Fs = [int(v) for v in rng.randint(1, Fmax + 1, size=B)]
    Fs[:4] = [1, 2, Fmax, Fmax - 1]
    amps = np.zeros((B, Fmax), dtype=np.int16)
    n_samples = []
    for b, F in enumerate(Fs):
        amps[b, :F] = K.random_amps(rng, F)
        n_samples.append(160 * F - int(rng.randint(0, 160)))
    wave = torch.from_numpy(amps).to(dev).repeat_interleave(160, dim=1)
    wave[:, 1::2] *= -1                                                      # the sign of a sample does not matter
    lens = torch.tensor(n_samples, dtype=torch.int32, device=dev)
    P = O.params(**K.SMALL)
    want_levels = [_frame_levels(amps[b], n_samples[b]) for b in range(B)]
    res = ops.vad_segments(wave, lens, max_segments=Fmax, return_levels=True, **K.SMALL)
    _assert_rows(res, want_levels, n_samples, P, Fmax)
    assert int(res.n_segs.max()) > 50 and int((res.n_segs == 0).sum()) < B // 4
    # the f32 form of the first rows, and other thresholds on the same levels
    sub = slice(0, 24)
    res_f = ops.vad_segments(wave[sub].float() / 32768.0, lens[sub], max_segments=Fmax, return_levels=True, **K.SMALL)
    assert torch.equal(res_f.levels, res.levels[sub]) and torch.equal(res_f.n_segs, res.n_segs[sub]) and torch.equal(res_f.floor, res.floor[sub])
    for b in range(24):
        assert torch.equal(res_f.segs[b, :int(res.n_segs[b])], res.segs[b, :int(res.n_segs[b])])
    other = dict(on_db=20.0, off_db=0.0, floor_permille=500, min_level_db=-80.0, max_floor_db=-20.0, min_silence_s=0.05, min_speech_s=0.03,
                 pad_s=0.04, max_segment_s=0.13)
    res_o = ops.vad_segments(wave[sub], lens[sub], max_segments=Fmax, return_levels=True, **other)
    _assert_rows(res_o, want_levels[sub], n_samples[sub], O.params(**other), Fmax)


def test_rows_of_different_lengths_in_a_wider_pitch(dev):
    from lightning_asr_amd import ops
    rng = np.random.RandomState(5)
    Fs, Fmax = [40, 17, 0], 40
    amps = np.zeros((3, Fmax), dtype=np.int16)
    for b, F in enumerate(Fs):
        amps[b, :F] = K.random_amps(rng, F) if F else 0
    n_samples = [160 * 40, 160 * 17 - 9, 0]
    L = 160 * Fmax
    big = torch.full((3, L + 37), 12345, dtype=torch.int16, device=dev)     # what lies past L, or past a row's length, is never read
    big[:, :L] = torch.from_numpy(amps).to(dev).repeat_interleave(160, dim=1)
    for b in range(3):
        big[b, n_samples[b]:L] = 20000
    wave = big[:, :L]
    assert wave.stride(0) == L + 37
    lens = torch.tensor(n_samples, dtype=torch.int32, device=dev)
    res = ops.vad_segments(wave, lens, max_segments=64, return_levels=True, **K.SMALL)
    _assert_rows(res, [_frame_levels(amps[b], n_samples[b]) for b in range(3)], n_samples, O.params(**K.SMALL), Fmax)
    assert int(res.n_segs[2]) == 0 and int(res.floor[2]) == 0


def test_max_segments_below_the_count_writes_the_first_rows_only(dev):
    from lightning_asr_amd import _lib, ops
    amps = np.array(([K.H] * 2 + [K.Z] * 5) * 9, dtype=np.int16)             # nine runs, seven frames apart
    wave = torch.from_numpy(O.amplitude_wave(amps)).to(dev)
    P = O.params(**K.SMALL)
    want, _ = O.segment_levels(_frame_levels(amps, wave.numel()), wave.numel(), P)
    assert want.shape[0] == 9
    segs = torch.full((9, 2), -7, dtype=torch.int32, device=dev)             # the call is told of 3 rows; the rest is the canary
    n_segs = torch.full((1,), -7, dtype=torch.int32, device=dev)
    p = ops.vad_params(**K.SMALL)
    nb = int(_lib.load().lasr_vad_workspace_bytes(1, wave.numel()))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.call("lasr_vad_segment", wave.data_ptr(), _lib.WAVE_PCM16, 0, None, 1, wave.numel(), ctypes.byref(p), segs.data_ptr(), 3,
              n_segs.data_ptr(), None, None, ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    assert int(n_segs) == 9                                                  # the true count
    assert torch.equal(segs[:3].cpu(), torch.from_numpy(want[:3])) and bool((segs[3:] == -7).all())
    res = ops.vad_segments(wave, max_segments=3, **K.SMALL)                  # the wrapper reports the same
    assert int(res.n_segs) == 9 and res.segs.shape == (3, 2) and torch.equal(res.segs.cpu(), torch.from_numpy(want[:3]))
    res0 = ops.vad_segments(wave, max_segments=0, **K.SMALL)
    assert int(res0.n_segs) == 9 and res0.segs.shape == (0, 2)


def test_speech_and_silence_alternating_at_every_frame(dev):
    """the longest run list a row can have: (F + 1) / 2 runs, more than one sweep of them"""
    from lightning_asr_amd import ops
    S = ops.vad_sweep()
    F = 2 * S + 1
    amps = np.zeros(F, dtype=np.int16)
    amps[0::2] = K.H
    wave = torch.from_numpy(amps).to(dev).repeat_interleave(160).unsqueeze(0)
    lev = _frame_levels(amps, 160 * F)
    single = dict(min_silence_s=0.01, min_speech_s=0.01, pad_s=0.0, max_segment_s=0.08)      # every run stays a segment of one frame
    res = ops.vad_segments(wave, max_segments=S + 1, return_levels=True, **single)
    assert int(res.n_segs[0]) == S + 1
    _assert_rows(res, [lev], [160 * F], O.params(**single), F)
    res = ops.vad_segments(wave, max_segments=F, return_levels=True, **K.SMALL)               # all closed into one run, then split
    _assert_rows(res, [lev], [160 * F], O.params(**K.SMALL), F)
    assert int(res.n_segs[0]) >= F // 8


def test_arguments_the_calls_refuse(dev):
    from lightning_asr_amd import _lib, ops
    wave = torch.zeros(1600, dtype=torch.int16, device=dev)
    with pytest.raises(_lib.LasrError):
        ops.vad_segments(wave.cpu())                                         # no CPU path
    with pytest.raises(_lib.LasrError):
        ops.vad_segments(wave.double())
    for bad in (dict(on_db=3.0, off_db=6.0), dict(floor_permille=0), dict(floor_permille=1001), dict(max_segment_s=0.01),
                dict(min_level_db=-10.0, max_floor_db=-20.0), dict(min_silence_s=float("nan")), dict(pad_s=-1.0), dict(on_db=float("inf"))):
        with pytest.raises(_lib.LasrError):
            ops.vad_segments(wave, **bad)
    with pytest.raises(ValueError):
        ops.vad_segments(wave, max_segments=-1)


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32], ids=["pcm16", "f32"])
def test_gather_copies_segments_and_zeroes_the_tails(dev, dtype):
    from lightning_asr_amd import ops
    g = torch.Generator().manual_seed(3)
    B, L = 3, 5000
    big = (torch.randint(-30000, 30000, (B, L + 11), generator=g).to(torch.int16) if dtype == torch.int16
           else torch.randn(B, L + 11, generator=g)).to(dev)
    wave = big[:, :L]                                                        # pitch > L
    table = [(0, 0, 1), (2, 4000, 5000), (1, 17, 2500), (0, 123, 123), (2, 0, 5000), (1, 4999, 5000)]     # the row's very end included
    rows, lens = ops.gather_segments(wave, table)
    assert rows.shape == (6, 5000) and rows.dtype == dtype and lens.tolist() == [e - s for _, s, e in table]
    for i, (r, s, e) in enumerate(table):
        assert torch.equal(rows[i, :e - s], wave[r, s:e]) and not rows[i, e - s:].any()
    rows2, lens2 = ops.gather_segments(wave, torch.tensor(table[:4], dtype=torch.int32), L_out=2483 + 300)   # a tensor table, a wider L_out
    assert rows2.shape == (4, 2783) and torch.equal(rows2[:, :2483], rows[:4, :2483]) and not rows2[:, 2483:].any()
    one, n1 = ops.gather_segments(wave[1], [(0, 5, 9)])                      # a 1-D wave is row 0
    assert torch.equal(one[0], wave[1, 5:9]) and n1.tolist() == [4]


def test_gather_more_segments_than_one_launch_carries(dev):
    from lightning_asr_amd import ops
    wave = torch.arange(0, 20000, dtype=torch.float32, device=dev)
    table = [(0, 7 * i, 7 * i + 1 + i % 13) for i in range(600)]
    rows, lens = ops.gather_segments(wave, table)
    assert rows.shape == (600, 13) and lens.tolist() == [1 + i % 13 for i in range(600)]
    want = torch.zeros(600, 13)
    for i, (_, s, e) in enumerate(table):
        want[i, :e - s] = torch.arange(s, e, dtype=torch.float32)
    assert torch.equal(rows.cpu(), want)


def test_gather_empty_table_and_refusals(dev):
    from lightning_asr_amd import _lib, ops
    wave = torch.ones(2, 1000, dtype=torch.int16, device=dev)
    rows, lens = ops.gather_segments(wave, [])
    assert rows.shape == (0, 0) and lens.shape == (0,)
    rows, lens = ops.gather_segments(wave, np.zeros((0, 3), dtype=np.int32), L_out=64)
    assert rows.shape == (0, 64) and rows.dtype == torch.int16
    with pytest.raises(_lib.LasrError, match=r"\(-2\).*out_pitch"):          # LASR_E_SHAPE: a segment wider than out_pitch
        ops.gather_segments(wave, [(0, 0, 10), (1, 100, 201)], L_out=100)
    for bad in ([(2, 0, 10)], [(-1, 0, 10)], [(0, 10, 5)], [(0, -1, 5)], [(0, 0, 1001)]):
        with pytest.raises(ValueError):
            ops.gather_segments(wave, bad)
    with pytest.raises(_lib.LasrError):
        ops.gather_segments(wave.cpu(), [(0, 0, 10)])
