"""CPU tier of the voice-activity segmenter: the numpy oracle (tests/helpers/vad_oracle.py - the rule of DESIGN.md "Inference: long
recordings", written independently of the library) against hand-written cases.  tests/test_gpu_vad.py then holds the kernels to
the oracle bit for bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vad_cases as K  # noqa: E402
import vad_oracle as O  # noqa: E402


def test_level_is_the_quasi_log_of_the_rule():
    assert [O.level(e) for e in (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 18)] == [0, 1, 9, 13, 17, 23, 25, 26, 32, 33, 33, 34]
    assert O.level(O.MAX_ENERGY) == 8 * 37 + 2 + 1 < O.LEVELS                 # 160 * 2^30 = 1.25 * 2^37
    es = sorted(set(max(0, (1 << k) + d) for k in range(39) for d in (-1, 0, 1)) | {O.MAX_ENERGY})
    lv = [O.level(e) for e in es]
    assert all(a <= b for a, b in zip(lv, lv[1:]))
    assert np.array_equal(O.levels_of_energy(es), np.array(lv, dtype=np.uint16))   # the vectorised form is the same function
    # one step is 10 log10(2) / 8 dB: a factor of two in power is eight levels
    assert O.level(1 << 20) - O.level(1 << 19) == 8 and abs(O.STEP_DB - 0.37629) < 1e-5


def test_parameter_conversion():
    P = O.params()
    assert P == {"on_steps": 32, "off_steps": 16, "floor_permille": 100, "min_level": 139, "max_floor_level": 205, "min_silence": 30,
                 "min_speech": 10, "pad": 10, "max_frames": 1600}
    S = O.params(**K.SMALL)
    assert (S["min_silence"], S["min_speech"], S["pad"], S["max_frames"]) == (3, 2, 1, 8)
    assert O.params(min_level_db=-1000.0)["min_level"] == 0 and O.params(max_floor_db=0.0)["max_floor_level"] == O.level(O.MAX_ENERGY)


def test_amplitudes_of_the_cases_have_the_levels_their_comments_state():
    lv = O.levels(O.amplitude_wave([K.Z, K.Q, K.M, K.H, K.L])).tolist()
    assert lv == [0, 137, 165, 190, 243]
    assert O.levels(O.amplitude_wave([K.L])[:1]).tolist() == [185]


@pytest.mark.parametrize("case", K.hand_cases(), ids=lambda c: c["name"])
def test_oracle_gives_the_hand_written_segments(case):
    P = O.params(**case["kwargs"])
    segs, floor, lev = O.segment(case["wave"], P)
    assert segs.dtype == np.int32 and segs.shape == (len(case["want"]), 2)
    assert [tuple(s) for s in segs.tolist()] == case["want"]
    assert lev.size == -(-case["wave"].size // 160)


def test_the_six_second_recording():
    pcm = O.recording_6s()
    P = O.params()
    segs, floor, lev = O.segment(pcm, P)
    want = [(int(round(a * 16000)), int(round(b * 16000))) for a, b in O.RECORDING_6S_SEGMENTS]
    assert [tuple(s) for s in segs.tolist()] == want                           # exact to the frame: every border is a frame border
    assert abs(floor - P["min_level"]) <= 8                                    # the noise at 0.001 is -60 dBFS, within a few steps
    # the PCM16 and f32 forms of one signal agree in every level and segment
    f32 = pcm.astype(np.float32) / np.float32(32768.0)
    segs_f, floor_f, lev_f = O.segment(f32, P)
    assert np.array_equal(lev, lev_f) and np.array_equal(segs, segs_f) and floor == floor_f


def test_f32_quantisation_rounds_half_to_even_and_saturates():
    x = np.array([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, 1.0, -1.0, 2.0, -3.0], dtype=np.float32)
    assert O.quantise(x).tolist() == [0, 2, 2, 0, 32767, -32768, 32767, -32768]


def test_split_pieces_are_ordered_and_never_longer_than_max_frames():
    rng = np.random.RandomState(7)
    P = O.params(**K.SMALL)
    for _ in range(50):
        lev = O.levels(O.amplitude_wave(K.random_amps(rng, 400)))
        fs, _ = O.frame_segments(lev, P)
        assert all(0 <= s < e <= 400 for s, e in fs) and all(a[1] <= b[0] for a, b in zip(fs, fs[1:]))
        assert all(e - s <= 8 for s, e in fs)
