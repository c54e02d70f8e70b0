"""Reference banded CTC forced alignment (the definition of lasr_ctc_align_long in include/lasr.h) in numpy, O(T * W).

The lattice, the emission rule, the max and its tie rule (stay, then step, then skip), the end rule and the outputs are those of
ctc_align_oracle (the full lattice); only a band of W states is alive per frame:

  frame t keeps states [lo_t, lo_t + W); lo_0 = 0; lo changes only at frames t0 that are positive multiples of R = 32.  There
    a      = the live (> -5e29, below 2S+1) state of row t0-1 with the largest value, the lowest such state; lo when none is live
    centre = floor((a - W/2) / G) * G                                     (G = 64)
    reach  = ceil((s_min(te) - (W-1)) / G) * G, te = min(t0 + R - 1, Tb - 1), s_min(t) = 2S-1 - 2 (Tb-1-t)
    lo     = min(max(lo_prev, centre, reach), ceil(max(0, 2S+1 - W) / G) * G)
  a candidate read from a state outside the PREVIOUS frame's band is dead; states >= 2S+1 are dead.

status: 0 aligned; 1 infeasible by count (Tb < S + adjacent equal labels, or Tb == 0 < S); 2 lost (feasible by count, neither
end state live).  On 1 and 2 the other outputs are the infeasible outputs of the full-lattice aligner.  band_lo follows the rule
for every frame below Tb whatever the status, and is -1 from Tb on.

One max and one f32 add per state per frame: a kernel that follows the definition agrees with this bit for bit."""
import numpy as np

import ctc_align_oracle as A

R = 32
G = 64
NINF = np.float32(-np.inf)
LIVE = np.float32(0.5) * A.K_DEAD


def n_repeats(target):
    return sum(1 for a, b in zip(target, target[1:]) if a == b)


def next_lo(lo_prev, a, t0, Tb, S, W):
    """the band origin of frames t0 .. t0+R-1 (plain integers; // is floor division)"""
    SS = 2 * S + 1
    te = min(t0 + R - 1, Tb - 1)
    s_min = 2 * S - 1 - 2 * (Tb - 1 - te)
    centre = ((a - W // 2) // G) * G
    reach = -((-(s_min - (W - 1))) // G) * G
    top = -((-max(0, SS - W)) // G) * G
    return min(max(lo_prev, centre, reach), top)


def align_long_one(logp, target, blank, band):
    """logp (Tb, C) f32, target: S labels -> (status, score f32, states (Tb,) i32 | None, band_lo (Tb,) i32)"""
    lp = np.asarray(logp, dtype=np.float32)
    Tb, S, W = lp.shape[0], len(target), int(band)
    assert W >= 256 and W % 256 == 0
    SS = 2 * S + 1
    by_count = 1 if (Tb < S + n_repeats(list(target)) or (Tb == 0 and S > 0)) else 0
    if Tb == 0:
        return by_count, (np.float32(0.0) if S == 0 else NINF), (np.zeros(0, np.int32) if S == 0 else None), np.zeros(0, np.int32)
    tg = np.asarray(target, dtype=np.int64)
    n_pad = SS + W + 2                                   # states the band may cover past 2S: blank class, never live
    cls = np.full(n_pad, blank, dtype=np.int64)
    cls[1:SS:2] = tg
    skip_ok = np.zeros(n_pad, dtype=bool)
    if S > 1:
        skip_ok[3:SS:2] = tg[1:] != tg[:-1]
    in_lat = np.arange(n_pad) < SS
    lo = 0
    band_lo = np.zeros(Tb, np.int32)
    v = np.full(W, NINF, dtype=np.float32)
    v[0] = lp[0, cls[0]]
    if SS > 1:
        v[1] = lp[0, cls[1]]
    back = np.zeros((Tb, W), dtype=np.int8)
    rel = np.arange(-2, W)
    with np.errstate(invalid="ignore"):
        for t in range(1, Tb):
            lo_prev = lo
            if t % R == 0:
                live = v > LIVE
                a = lo_prev + int(np.argmax(np.where(live, v, NINF))) if live.any() else lo_prev
                lo = next_lo(lo_prev, a, t, Tb, S, W)
            band_lo[t] = lo
            idx = rel + (lo - lo_prev)                   # states lo-2 .. lo+W-1 as positions of the previous band
            ok = (idx >= 0) & (idx < W)
            ext = np.where(ok, v[np.clip(idx, 0, W - 1)], NINF).astype(np.float32)
            st = slice(lo, lo + W)
            stay, step = ext[2:], ext[1:-1]
            skip = np.where(skip_ok[st], ext[:-2], NINF).astype(np.float32)
            m = np.maximum(np.maximum(stay, step), skip)
            back[t] = np.where(stay == m, 0, np.where(step == m, 1, 2))
            v = np.where(in_lat[st], (m + lp[t, cls[st]]).astype(np.float32), NINF).astype(np.float32)

    def at(s):
        return v[s - lo] if lo <= s < lo + W and s >= 0 else NINF
    v_blank, v_label = at(SS - 1), at(SS - 2)
    end = SS - 1 if (S == 0 or v_blank >= v_label) else SS - 2
    score = at(end)
    if not (score > LIVE):
        return (1 if by_count else 2), NINF, None, band_lo
    states = np.zeros(Tb, dtype=np.int32)
    s = end
    for t in range(Tb - 1, 0, -1):
        states[t] = s
        s = max(s - int(back[t, s - band_lo[t]]), 0)
    states[0] = s
    return 0, np.float32(score), states, band_lo


def align_long_batch(logp, targets, in_lens, tgt_lens, blank, band):
    """as ctc_align_oracle.align_batch, + status (B) i32 and band_lo (B, T) i32"""
    lp = np.asarray(logp, dtype=np.float32)
    B, T, C = lp.shape
    targets = np.asarray(targets, dtype=np.int64)
    targets = targets if targets.ndim == 2 else targets.reshape(B, 0)
    S_max = targets.shape[1]
    score = np.zeros(B, np.float32)
    frame_state = np.full((B, T), -1, np.int32)
    frame_logp = np.zeros((B, T), np.float32)
    label_start = np.full((B, S_max), -1, np.int32)
    label_end = np.full((B, S_max), -1, np.int32)
    status = np.zeros(B, np.int32)
    band_lo = np.full((B, T), -1, np.int32)
    for b in range(B):
        Tb = T if in_lens is None else int(min(max(int(in_lens[b]), 0), T))
        S = int(min(max(int(tgt_lens[b]), 0), S_max))
        tg = np.clip(targets[b, :S], 0, C - 1)
        status[b], score[b], st, band_lo[b, :Tb] = align_long_one(lp[b, :Tb], tg.tolist(), blank, band)
        if st is None:
            continue
        frame_state[b, :Tb] = st
        odd = (st & 1) == 1
        c = np.where(odd, tg[np.minimum(st >> 1, max(S - 1, 0))] if S else blank, blank)
        frame_logp[b, :Tb] = lp[b, np.arange(Tb), c]
        prev = np.concatenate(([-1], st[:-1]))
        nxt = np.concatenate((st[1:], [-1]))
        t = np.arange(Tb)
        opens, closes = odd & (prev != st), odd & (nxt != st)
        label_start[b, st[opens] >> 1] = t[opens]
        label_end[b, st[closes] >> 1] = t[closes] + 1
    return score, frame_state, frame_logp, label_start, label_end, status, band_lo


def log_softmax(x):
    x = np.asarray(x, dtype=np.float32)
    x = x - x.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        return (x - np.log(np.exp(x.astype(np.float64)).sum(axis=1, keepdims=True))).astype(np.float32)


def plant_path(labels, T, blank, rng):
    """a random monotone frame labelling of T frames that collapses to `labels`: every label >= 1 frame, a blank between equal
    neighbours, the spare frames spread at random over the entries and the gaps between them"""
    seq = []                                             # the shortest class sequence
    for i, c in enumerate(labels):
        if i and labels[i - 1] == c:
            seq.append(blank)
        seq.append(int(c))
    assert len(seq) <= T, "plant_path: T too short"
    extra = np.bincount(rng.randint(0, 2 * len(seq) + 1, size=T - len(seq)), minlength=2 * len(seq) + 1)
    path = []
    for j, c in enumerate(seq):
        path.extend([blank] * int(extra[2 * j]))         # blank frames in the gap before entry j
        path.extend([c] * (1 + int(extra[2 * j + 1])))
    path.extend([blank] * int(extra[2 * len(seq)]))
    assert len(path) == T
    return np.asarray(path, dtype=np.int64)


def planted(T, S, C, hot, seed):
    """labels uniform in [0, C-1), a planted alignment (plant_path), logp = log_softmax(N(0,1) + hot at the planted class).
    -> (logp (T, C) f32, labels (S,) i64)"""
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, C - 1, size=S).astype(np.int64)
    path = plant_path(labels.tolist(), T, C - 1, rng)
    x = rng.standard_normal((T, C)).astype(np.float32)
    x[np.arange(T), path] += np.float32(hot)
    return log_softmax(x), labels


def lost_case(seed=0):
    """T = 800, S = 300, C = 28.  Label 200 is class 0 and no other label is.  Frames 0..399 are random with blank + 8; frames
    400.. carry a planted path for labels 201.. with class 0 at -inf: label 200 has to be spoken in the first half, where nothing
    pulls the band towards it.  -> (logp, labels)"""
    T, S, C, half = 800, 300, 28, 400
    rng = np.random.RandomState(seed)
    labels = rng.randint(1, C - 1, size=S).astype(np.int64)
    labels[200] = 0
    x = rng.standard_normal((T, C)).astype(np.float32)
    x[:half, C - 1] += np.float32(8.0)
    path = plant_path(labels[201:].tolist(), T - half, C - 1, rng)
    x[half + np.arange(T - half), path] += np.float32(4.0)
    x[half:, 0] = -np.inf
    return log_softmax(x), labels


def tight_case(seed=0):
    """T = 420, S = 400, labels i % 5, blank-favoured frames: only `reach` takes the band to the end in time.  -> (logp, labels)"""
    T, S, C = 420, 400, 28
    rng = np.random.RandomState(seed)
    labels = (np.arange(S) % 5).astype(np.int64)
    x = rng.standard_normal((T, C)).astype(np.float32)
    x[:, C - 1] += np.float32(4.0)
    return log_softmax(x), labels
