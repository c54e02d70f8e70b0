"""f64 oracle of the weight EMA ("Weight EMA"): the recurrence e <- e + (p - e) w in float64 over a given sequence of
parameter vectors, with the decay warm-up restated in plain Python floats.  The tests feed it the GPU's own parameter sequence, so
that the difference to the GPU's f32 average is the average's rounding alone."""
from typing import Iterable, List, Tuple

import numpy as np


def decay_at(decay: float, warmup: bool, t: int) -> float:
    """the decay of update number t (0-based), exact up to one float64 division"""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def recurrence(e0: np.ndarray, params: Iterable[np.ndarray], weights: Iterable[float]) -> Tuple[np.ndarray, List[np.ndarray]]:
    """e0: the average's start; params[k]: the parameters after step k; weights[k]: the weight w = 1 - d of update k (the f32 value
    the device used, so that the oracle isolates the three roundings of the update from the one of the weight).
    Returns (the final average, the average after every step), float64."""
    e = np.asarray(e0, dtype=np.float64).copy()
    trace = []
    for p, w in zip(params, weights):
        e = e + (np.asarray(p, dtype=np.float64) - e) * float(w)
        trace.append(e.copy())
    return e, trace


def drift_bound(max_abs: float, d_max: float) -> float:
    """|e_f32 - e_f64| per element after any number of updates.  One update rounds three times: the difference (|p - e| <= 2 M, half
    an ulp <= 2^-24 * 2 M), the product (|w diff| <= 2 M: again <= 2 M 2^-24) and the sum (|e| <= M: <= M 2^-24), at most
    5 M 2^-24 in all; the error already in e is multiplied by d = 1 - w <= d_max by every later update, so the errors sum to at
    most 5 M 2^-24 (1 + d_max + d_max^2 + ...) = 5 M 2^-24 / (1 - d_max)."""
    return 5.0 * 2.0 ** -24 * float(max_abs) / (1.0 - float(d_max))
