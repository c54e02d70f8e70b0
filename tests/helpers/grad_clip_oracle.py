"""f64 oracle of the optimiser step with gradient clipping and the non-finite guard ("Gradient clipping and the non-finite
guard"): NovoGrad over a tensor table (flat buffers + an offset list) in plain numpy float64, with both clips and the guard as the
specification words them.  Nothing here is rounded to f32: the tests compare the GPU's f32 step against it."""
from typing import Dict, Sequence

import numpy as np


def clip_coef(total_norm: float, c: float) -> float:
    """min(1, c / (N + 1e-6)) - the constants of torch.nn.utils.clip_grad_norm_; a NaN stays a NaN"""
    with np.errstate(all="ignore"):
        q = np.float64(c) / (np.float64(total_norm) + 1e-6)
    return 1.0 if q > 1.0 else float(q)


def step(state: Dict[str, np.ndarray], grad: np.ndarray, offsets: Sequence[int], lr: float, beta1: float = 0.8, beta2: float = 0.5,
         eps: float = 1e-8, weight_decay: float = 0.0, grad_scale: float = 1.0, algorithm: str = "off", clip_val: float = 0.0,
         skip_nonfinite: bool = False) -> Dict[str, float]:
    """One step, in place.  state: {"p": (n,), "m": (n,), "v": (n_tensors,)} float64.  Returns {"total_norm", "coef", "skipped"}:
    total_norm is the global norm of the scaled gradient before the norm clip (value mode: of the clamped values)."""
    if algorithm not in ("off", "norm", "value"):
        raise ValueError(algorithm)
    g = np.asarray(grad, dtype=np.float64) * float(grad_scale)
    if algorithm == "value":
        with np.errstate(all="ignore"):
            g = np.where(g < -clip_val, -clip_val, np.where(g > clip_val, clip_val, g))        # NaN stays NaN, +-Inf -> +-c
    n_t = len(offsets) - 1
    with np.errstate(all="ignore"):
        norm2 = np.array([np.sum(g[offsets[t]:offsets[t + 1]] ** 2) for t in range(n_t)], dtype=np.float64)
        total2 = float(np.sum(norm2))
        total_norm = float(np.sqrt(total2))
    coef = clip_coef(total_norm, clip_val) if algorithm == "norm" else 1.0
    if skip_nonfinite and not np.isfinite(total2):
        return {"total_norm": total_norm, "coef": coef, "skipped": True}
    with np.errstate(all="ignore"):
        g = g * coef
        norm2 = norm2 * coef * coef
        v = state["v"]
        v[:] = np.where(v == 0.0, norm2, beta2 * v + (1.0 - beta2) * norm2)
        denom = np.sqrt(v) + eps
        p, m = state["p"], state["m"]
        for t in range(n_t):
            lo, hi = offsets[t], offsets[t + 1]
            gi = g[lo:hi] / denom[t]
            if weight_decay != 0.0:
                gi = gi + weight_decay * p[lo:hi]
            m[lo:hi] = m[lo:hi] * beta1 + gi
            p[lo:hi] = p[lo:hi] - lr * m[lo:hi]
    return {"total_norm": total_norm, "coef": coef, "skipped": False}
