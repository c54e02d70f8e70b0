"""Hand-written cases of the segmentation rule, shared by tests/test_host_vad.py (the oracle against them) and
tests/test_gpu_vad.py (the kernels against the oracle).  A case is frames of constant int16 amplitude, so its levels are known:
Z = 0 (level 0), Q = 30 (below `off`), M = 100 (between `off` and `on`), H = 300 and L = 3000 (above `on`), with the floor at
its lower clamp (min_level_db = -60: level 139, off = 155, on = 171).  SMALL are the parameters that make every pass work at a
handful of frames: min_silence 3, min_speech 2, pad 1, max_frames 8."""
import numpy as np

import vad_oracle as O

Z, Q, M, H, L = 0, 30, 100, 300, 3000
SMALL = dict(min_silence_s=0.03, min_speech_s=0.02, pad_s=0.01, max_segment_s=0.08)


def _case(name, amps, want_frames, n_samples=None, **kw):
    wave = O.amplitude_wave(amps)
    if n_samples is not None:
        wave = wave[:n_samples]
    args = dict(SMALL)
    args.update(kw)
    n = wave.size
    return {"name": name, "wave": wave, "kwargs": args, "want": [(160 * s, min(160 * e, n)) for s, e in want_frames]}


def hand_cases():
    c = []
    c.append(_case("all_zero", [Z] * 20, []))
    c.append(_case("quiet_only", [Q] * 20, []))
    c.append(_case("mid_never_reaches_on", [Z] * 3 + [M] * 5 + [Z] * 3, []))
    c.append(_case("hysteresis_keeps_the_mid_skirt", [Z] * 3 + [M, M, H, M] + [Z] * 4, [(2, 8)]))
    # gap of min_silence - 1 = 2 closes, gap of min_silence = 3 stays: runs [1,3) [5,7) [10,12)
    c.append(_case("gap", [Z, H, H, Z, Z, H, H, Z, Z, Z, H, H, Z, Z, Z, Z], [(0, 8), (9, 13)]))
    # a run of min_speech - 1 = 1 is dropped, one of min_speech = 2 stays
    c.append(_case("short_run", [Z] * 3 + [H] + [Z] * 5 + [H, H] + [Z] * 3, [(8, 12)]))
    # pad 2: runs [3,5) [9,11) pad to [1,7) [7,13), which touch and merge; [16,18) pads to [14,20), one frame clear.  The merged
    # run of 12 frames is cut at the first of the four level-0 frames of its window [5, 9)
    c.append(_case("pads_touch", [Z] * 3 + [H] * 2 + [Z] * 4 + [H] * 2 + [Z] * 5 + [H] * 2 + [Z] * 3, [(1, 5), (5, 13), (14, 20)], pad_s=0.02))
    # padded runs of max_frames = 8 and of 9 frames; the 9 is cut at the first frame of an all-equal window [16, 20)
    c.append(_case("max_frames", [Z] * 2 + [H] * 6 + [Z] * 5 + [H] * 7 + [Z] * 2, [(1, 9), (12, 16), (16, 21)]))
    # the single lowest frame of the window [5, 9) is frame 7
    c.append(_case("split_at_the_lowest", [Z] * 2 + [H] * 5 + [M] + [H] * 3 + [Z] * 2, [(1, 7), (7, 12)]))
    # the first and the last frame are speech: the pad is clipped to the row, the silence outside is never closed
    c.append(_case("edges", [H, H] + [Z] * 6 + [H, H], [(0, 3), (7, 10)]))
    # one constant loud tone from end to end: the floor is the tone itself, max_floor_db (level 205) keeps `on` (237) below it (243)
    c.append(_case("loud_from_end_to_end", [L] * 6, [(0, 6)]))
    c.append(_case("constant_but_not_loud", [H] * 6, []))
    # lengths around one frame, min_speech 1: a lone sample (level 185) is its own floor and no speech; 159 and 160 samples are one
    # loud frame; at 161 the one-sample frame is the floor, frame 0 is speech and the pad takes the row's last sample in
    c.append(_case("len_0", [L], [], n_samples=0, min_speech_s=0.01))
    c.append(_case("len_1", [L], [], n_samples=1, min_speech_s=0.01))
    c.append(_case("len_159", [L], [(0, 1)], n_samples=159, min_speech_s=0.01))
    c.append(_case("len_160", [L], [(0, 1)], n_samples=160, min_speech_s=0.01))
    c.append(_case("len_161", [L, L], [(0, 2)], n_samples=161, min_speech_s=0.01))
    return c


def random_amps(rng: np.random.RandomState, F: int) -> np.ndarray:
    """a level pattern of F frames: stretches of one amplitude, their lengths around the small parameters"""
    out = np.zeros(F, dtype=np.int16)
    n = 0
    while n < F:
        k = int(rng.choice([1, 1, 2, 2, 3, 4, 5, 7, 9, 13, 30]))
        out[n:n + k] = rng.choice([Z, Z, Q, M, H, H, L])
        n += k
    return out
