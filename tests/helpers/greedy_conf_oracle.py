"""Plain numpy / math.fsum restatement of lasr_greedy_confidence (include/lasr.h), written from its text: frame maxima with the
lowest-id tie rule, the greedy CTC collapse with the run of every token, per-token and per-utterance sums taken EXACTLY in f64
(math.fsum), the two utterance confidences.  Also the seeded inputs the golden file and the tests regenerate, and the ulp
distance the gates are stated in."""
from __future__ import annotations

import math

import numpy as np


def make_logp(seed: int, B: int, T: int, C: int, blank: int, blank_bias: float = 0.0, scale: float = 2.0) -> np.ndarray:
    """(B, T, C) f32 log-probs from a seed: normal logits times `scale`, `blank_bias` added to the blank's (so that the blank
    wins a good share of the frames), log-softmax taken in f64 and rounded once to f32"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, C)).astype(np.float64) * scale
    x[:, :, blank] += blank_bias
    x -= x.max(-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def frame_stats(rows: np.ndarray):
    """(m, a) of the frames (T, C): the maximum and the lowest class attaining it; a row of -inf only gives (-inf, 0)"""
    m = rows.max(-1)
    return m, np.argmax(rows == m[:, None], -1)          # (argmax of booleans: the first True)


def confidence(total: float, n: int) -> float:
    """-( -1e-5 + total ) / ( n + 1e-6 ) in f64 with IEEE rules for -inf"""
    return float(-(np.float64(-1e-5) + np.float64(total)) / (np.float64(n) + np.float64(1e-6)))


def oracle(logp: np.ndarray, lens, blank: int) -> dict:
    B, T, C = logp.shape
    out = {"tokens": np.full((B, T), -1, np.int32), "n_tokens": np.zeros(B, np.int32), "tok_start": np.full((B, T), -1, np.int32),
           "tok_end": np.full((B, T), -1, np.int32), "tok_min": np.zeros((B, T), np.float32), "tok_mean": np.zeros((B, T), np.float64),
           "utt_sum": np.zeros((B, 2), np.float64), "n_nonblank": np.zeros(B, np.int32), "conf": np.zeros((B, 2), np.float64)}
    for b in range(B):
        Tb = T if lens is None else min(max(int(lens[b]), 0), T)
        m, a = frame_stats(logp[b, :Tb])
        m, a = [float(v) for v in m], [int(v) for v in a]
        i = 0
        t = 0
        while t < Tb:
            e = t + 1
            while e < Tb and a[e] == a[t]:
                e += 1
            if a[t] != blank:            # the run's first frame emits: t == 0 or a[t] != a[t-1] by construction of the runs
                out["tokens"][b, i] = a[t]
                out["tok_start"][b, i], out["tok_end"][b, i] = t, e
                out["tok_min"][b, i] = np.float32(min(m[t:e]))
                out["tok_mean"][b, i] = math.fsum(m[t:e]) / (e - t)
                i += 1
            t = e
        out["n_tokens"][b] = i
        lab = [m[t] for t in range(Tb) if a[t] != blank]
        out["utt_sum"][b] = (math.fsum(m), math.fsum(lab))
        out["n_nonblank"][b] = len(lab)
        out["conf"][b] = (confidence(out["utt_sum"][b, 0], Tb), confidence(out["utt_sum"][b, 1], len(lab)))
    return out


def ulp_distance(got_f32: np.ndarray, want_f64: np.ndarray) -> np.ndarray:
    """units in the last place between f32 values and f64 values rounded to f32 (0 where both are the same infinity)"""
    got = np.ascontiguousarray(got_f32, dtype=np.float32)
    want = np.ascontiguousarray(np.asarray(want_f64, dtype=np.float64).astype(np.float32))

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(got) - ordered(want))


def rel_err(got, want) -> float:
    """largest |got - want| / |want| over the finite entries (the others must agree exactly)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin])
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), np.finfo(np.float64).tiny)))
