"""numpy f64 oracle of the resampler (DESIGN.md "Resampling"), written from the definition and independent of csrc/resample.h:

    g = gcd(sr_in, sr_out); down = sr_in / g; up = sr_out / g; base = min(up, down) * rolloff
    width = ceil(lpw * down / base); taps = 2 * width + down
    h[p][k] = (base / down) * sinc(t) * cos(pi t / (2 lpw))^2,   t = clamp(((k - width) / down - p / up) * base, -lpw, lpw)
    n_out = ceil(n_in * up / down);  out[j] = sum_k h[j % up][k] * x[(j / up) * down + k - width],  x = 0 outside [0, n_in)

``resample`` returns, per output sample, the value y and A = sum_k |h x| - the scale of the rounding-error bounds the tests derive."""
import math

import numpy as np


def geometry(sr_in, sr_out, lpw=6, rolloff=0.99):
    """(up, down, width, taps)"""
    g = math.gcd(int(sr_in), int(sr_out))
    down, up = int(sr_in) // g, int(sr_out) // g
    base = min(up, down) * rolloff
    width = int(math.ceil(lpw * down / base))
    return up, down, width, 2 * width + down


def taps(sr_in, sr_out, lpw=6, rolloff=0.99):
    """h (up, taps) f64"""
    up, down, width, n = geometry(sr_in, sr_out, lpw, rolloff)
    base = min(up, down) * rolloff
    k = np.arange(n, dtype=np.float64)[None, :]
    p = np.arange(up, dtype=np.float64)[:, None]
    t = np.clip(((k - width) / down - p / up) * base, -float(lpw), float(lpw))
    window = np.cos(np.pi * t / (2.0 * lpw)) ** 2
    safe = np.where(t == 0.0, 1.0, t)
    sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))
    return (base / down) * sinc * window


def out_len(n_in, up, down):
    return -((-int(n_in) * int(up)) // int(down))


def resample(x, sr_in, sr_out, lpw=6, rolloff=0.99, h=None):
    """x (n,) -> (y (n_out,), A (n_out,)) in f64.  h: the taps to use instead of the exact ones (e.g. their f32 roundings)."""
    up, down, width, n_taps = geometry(sr_in, sr_out, lpw, rolloff)
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[0]
    n_out = out_len(n_in, up, down)
    if up == 1 and down == 1:                         # identity: a copy, the filter is not run
        return x.copy(), np.abs(x)
    h = taps(sr_in, sr_out, lpw, rolloff) if h is None else np.asarray(h, dtype=np.float64)
    assert h.shape == (up, n_taps)
    n_blocks = -(-n_out // up) if n_out else 0
    xp = np.zeros(width + n_blocks * down + n_taps, dtype=np.float64)      # x with `width` zeros in front and enough behind
    xp[width:width + n_in] = x
    y = np.zeros(n_blocks * up, dtype=np.float64)
    a = np.zeros(n_blocks * up, dtype=np.float64)
    if n_blocks:
        win = np.lib.stride_tricks.sliding_window_view(xp, n_taps)[::down][:n_blocks]    # (n_blocks, taps): x[q * down + k - width]
        for p in range(up):
            prod = win * h[p][None, :]
            y[p::up] = prod.sum(axis=1)
            a[p::up] = np.abs(prod).sum(axis=1)
    return y[:n_out], a[:n_out]
