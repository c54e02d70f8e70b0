"""The voice-activity segmentation rule (DESIGN.md "Inference: long recordings") in numpy and plain Python, independent of the
library: its own parameter conversion, its own level function, the passes written as the sequential walks the rule states (the
kernel runs them as scans).  Integer arithmetic throughout, so the kernel has to agree exactly.

    P = params(on_db=..., ...)                 # dict of the nine integers, from dB and seconds
    segs, floor, lev = segment(x, P)           # x: 1-D int16 or float32; segs (n, 2) int32 in samples
"""
import math

import numpy as np

HOP = 160
LEVELS = 512
STEP_DB = 10.0 * math.log10(2.0) / 8.0
MAX_ENERGY = HOP * 32768 ** 2


def level(e: int) -> int:
    e = int(e)
    if e == 0:
        return 0
    k = e.bit_length() - 1
    m = ((e >> (k - 3)) if k >= 3 else (e << (3 - k))) & 7
    return 8 * k + m + 1


def params(on_db=12.0, off_db=6.0, floor_permille=100, min_level_db=-60.0, max_floor_db=-35.0, min_silence_s=0.3, min_speech_s=0.1,
           pad_s=0.1, max_segment_s=16.0) -> dict:
    """Python's round() is half to even, as the rule asks"""
    def frames(s):
        return int(round(s * 100.0))

    def abs_level(db):
        return level(int(round(MAX_ENERGY * 10.0 ** (db / 10.0))))

    return {"on_steps": int(round(on_db / STEP_DB)), "off_steps": int(round(off_db / STEP_DB)), "floor_permille": int(floor_permille),
            "min_level": abs_level(min_level_db), "max_floor_level": abs_level(max_floor_db), "min_silence": frames(min_silence_s),
            "min_speech": frames(min_speech_s), "pad": frames(pad_s), "max_frames": frames(max_segment_s)}


def quantise(x) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.int64)
    if x.dtype != np.float32:
        raise TypeError("int16 or float32")
    return np.clip(np.rint(x * np.float32(32768.0)), -32768.0, 32767.0).astype(np.int64)


def levels(x) -> np.ndarray:
    """(F,) uint16 levels of a 1-D wave"""
    q = quantise(x)
    n = q.size
    F = -(-n // HOP)
    if F == 0:
        return np.zeros(0, dtype=np.uint16)
    sq = np.zeros(F * HOP, dtype=np.int64)
    sq[:n] = q * q
    return levels_of_energy(sq.reshape(F, HOP).sum(axis=1))


def levels_of_energy(E) -> np.ndarray:
    E = np.asarray(E, dtype=np.int64)
    out = np.zeros(E.shape, dtype=np.int64)
    nz = E > 0
    e = E[nz]
    k = np.frexp(e.astype(np.float64))[1].astype(np.int64) - 1          # exact: E < 2^53
    m = np.where(k >= 3, e >> np.maximum(k - 3, 0), e << np.maximum(3 - k, 0)) & 7
    out[nz] = 8 * k + m + 1
    return out.astype(np.uint16)


def noise_floor(lev: np.ndarray, permille: int) -> int:
    F = lev.size
    if F == 0:
        return 0
    rank = max(1, -(-F * permille // 1000))
    return int(np.sort(lev.astype(np.int64), kind="stable")[rank - 1])


def _runs(mask: np.ndarray):
    d = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def frame_segments(lev: np.ndarray, P: dict):
    """(list of (s, e) in frames, floor) for one row's levels"""
    lev = np.asarray(lev).astype(np.int64)
    F = lev.size
    floor = noise_floor(lev, P["floor_permille"])
    base = min(max(floor, P["min_level"]), P["max_floor_level"])
    on, off = base + P["on_steps"], base + P["off_steps"]
    runs = [(s, e) for s, e in _runs(lev >= off) if (lev[s:e] >= on).any()]           # hysteresis
    closed = []
    for s, e in runs:                                                                 # close
        if closed and s - closed[-1][1] < P["min_silence"]:
            closed[-1] = (closed[-1][0], e)
        else:
            closed.append((s, e))
    opened = [(s, e) for s, e in closed if e - s >= P["min_speech"]]                  # open
    padded = []
    for s, e in opened:                                                               # pad
        s, e = max(0, s - P["pad"]), min(F, e + P["pad"])
        if padded and s <= padded[-1][1]:
            padded[-1] = (padded[-1][0], e)
        else:
            padded.append((s, e))
    out, mf = [], P["max_frames"]
    for s, e in padded:                                                               # split
        while e - s > mf:
            lo = s + mf // 2
            c = lo + int(np.argmin(lev[lo:s + mf]))                                   # argmin: the first of the lowest
            out.append((s, c))
            s = c
        out.append((s, e))
    return out, floor


def segment_levels(lev: np.ndarray, n_samples: int, P: dict):
    fs, floor = frame_segments(lev, P)
    segs = np.array([(HOP * s, min(HOP * e, n_samples)) for s, e in fs], dtype=np.int32).reshape(-1, 2)
    return segs, floor


def segment(x, P: dict):
    lev = levels(x)
    segs, floor = segment_levels(lev, np.asarray(x).size, P)
    return segs, floor, lev


def amplitude_wave(amps) -> np.ndarray:
    """frames of constant amplitude: int16 wave of 160 * len(amps) samples whose frame n has E = 160 * amps[n]^2"""
    return np.repeat(np.asarray(amps, dtype=np.int16), HOP)


def recording_6s(seed: int = 0, rate: int = 16000) -> np.ndarray:
    """the hand case: 6 s (at 16 kHz unless told otherwise), a noise floor at 0.001 and tone bursts at 0.5-1.5 s, 1.6-2.0 s,
    3.0-3.05 s and 4.0-5.63 s; int16"""
    g = np.random.RandomState(seed)
    n = 6 * rate
    t = np.arange(n) / float(rate)
    y = 0.001 * g.standard_normal(n)
    tone = 0.3 * np.sin(2 * math.pi * 440.0 * t)
    for a, b in ((0.5, 1.5), (1.6, 2.0), (3.0, 3.05), (4.0, 5.63)):
        y[int(round(a * rate)):int(round(b * rate))] += tone[int(round(a * rate)):int(round(b * rate))]
    return np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)


RECORDING_6S_SEGMENTS = [(0.4, 2.1), (3.9, 5.73)]
