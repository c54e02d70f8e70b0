"""numpy f64 oracle of the noise and reverberation augmentation (DESIGN.md "Noise and reverberation"), written from the definition
and independent of csrc/wave_aug.h:

    RIR h:  d = first index of max |h|;  K = the smallest length >= d + 1 with sum_{k >= K} h[k]^2 <= 1e-6 sum_k h[k]^2, at most 8192
            (both sums in f64, accumulated from the last sample towards the first)
    reverb  y[j] = sum_{k < K} h[k] x[j + d - k], x = 0 outside [0, n), j in [0, n);   no reverb: y = x
    noise   v[j] = clip[(s + j) mod len];   no noise: v = 0
    E_x, E_y, E_n = sums of squares over [0, n);  g_s = sqrt(E_x / E_y) (1 without reverb, 0 if E_y == 0)
    g_n = sqrt(E_x / (E_n 10^(snr_cdb / 1000))) (0 without noise, or if E_x == 0 or E_n == 0)
    out = g_s y + g_n v

``fir`` also returns A[j] = sum_k |h[k] x[j + d - k]|, the scale of the rounding-error bounds the tests derive."""
import numpy as np

MAX_TAPS = 8192
TAIL = 1e-6


def rir_geometry(h):
    """(d, K) of one RIR"""
    h = np.asarray(h, dtype=np.float64)
    d = int(np.argmax(np.abs(h)))                       # argmax returns the first maximum
    tail = np.cumsum((h * h)[::-1])[::-1]               # tail[K] = sum_{k >= K}, accumulated from the end
    thr = TAIL * tail[0]
    ok = np.nonzero(np.append(tail, 0.0)[d + 1:] <= thr)[0]      # lengths d + 1 .. len; the full length always qualifies
    K = d + 1 + int(ok[0])
    return d, min(K, MAX_TAPS)


def fir(x, h, d, emulate_f32=False):
    """x (n,), taps h (K,), delay d -> (y (n,), A (n,)).  emulate_f32: every product and every partial sum rounded to f32, taps
    in ascending order - the arithmetic of a plain f32 loop, as the yardstick of the second FIR gate."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n, K = x.size, h.size
    xp = np.zeros(n + 2 * K, dtype=np.float64)          # xp[i] = x[i - K]
    xp[K:K + n] = x
    if emulate_f32:
        acc = np.zeros(n, dtype=np.float32)
        xf = xp.astype(np.float32)
        for k in range(K):
            acc = acc + np.float32(h[k]) * xf[K + d - k:K + d - k + n]
        return acc.astype(np.float64), None
    y = np.zeros(n, dtype=np.float64)
    a = np.zeros(n, dtype=np.float64)
    for k in range(K):
        seg = h[k] * xp[K + d - k:K + d - k + n]
        y += seg
        a += np.abs(seg)
    return y, a


def noise_row(clip, start, n):
    clip = np.asarray(clip, dtype=np.float64)
    return clip[(int(start) + np.arange(n, dtype=np.int64)) % clip.size]


def gains(ex, ey, en, reverb, noise, snr_cdb):
    gs = (np.sqrt(ex / ey) if ey > 0 else 0.0) if reverb else 1.0
    gn = np.sqrt(ex / (en * 10.0 ** (snr_cdb / 1000.0))) if (noise and ex > 0 and en > 0) else 0.0
    return float(gs), float(gn)


def augment(x, h=None, d=0, clip=None, start=0, snr_cdb=0):
    """x (n,) f64; h: taps (already cut to K) or None; clip: noise clip (f64) or None ->
    dict(out, y, v, A, stats = (E_x, E_y, E_n), gains = (g_s, g_n))"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    if h is not None:
        y, a = fir(x, h, d)
    else:
        y, a = x.copy(), np.abs(x)
    v = noise_row(clip, start, n) if clip is not None else np.zeros(n)
    ex, ey, en = float((x * x).sum()), float((y * y).sum()), float((v * v).sum())
    gs, gn = gains(ex, ey, en, h is not None, clip is not None, snr_cdb)
    return dict(out=gs * y + gn * v, y=y, v=v, A=a, stats=(ex, ey, en), gains=(gs, gn))
