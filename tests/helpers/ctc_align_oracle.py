"""Reference CTC forced alignment (the definition of lasr_ctc_align in include/lasr.h) as a numpy dynamic programme.

Scores are float32, dead states are -inf, one rounding per state per frame (max of the candidates, then one f32 add of the
emission).  The backpointer is the candidate that attains the max; on equality stay, then step, then skip.  The path ends in
state 2S when v[2S] >= v[2S-1] (or S == 0), else in 2S-1.  A final score that is not above 0.5 * kDead = -5e29 (-inf, NaN) is
infeasible: score -inf, every index output -1, frame_logp 0.

Because the recursion is a max and one add, a kernel that follows the definition agrees with this bit for bit."""
import itertools

import numpy as np

K_DEAD = np.float32(-1e30)


def align_one(logp, target, blank):
    """logp (Tb, C) f32, target: list of S labels -> (score f32, states (Tb,) i32 or None when infeasible)"""
    lp = np.asarray(logp, dtype=np.float32)
    Tb, S = lp.shape[0], len(target)
    SS = 2 * S + 1
    if Tb == 0:
        return (np.float32(0.0), np.zeros(0, np.int32)) if S == 0 else (np.float32(-np.inf), None)
    tg = np.asarray(target, dtype=np.int64)
    cls = np.full(SS, blank, dtype=np.int64)
    cls[1::2] = tg
    skip_ok = np.zeros(SS, dtype=bool)
    for s in range(3, SS, 2):
        skip_ok[s] = tg[s >> 1] != tg[(s >> 1) - 1]
    ninf = np.float32(-np.inf)
    v = np.full(SS, ninf, dtype=np.float32)
    v[0] = lp[0, cls[0]]
    if SS > 1:
        v[1] = lp[0, cls[1]]
    back = np.zeros((Tb, SS), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, Tb):
            stay = v
            step = np.concatenate(([ninf], v[:-1])).astype(np.float32)
            skip = np.where(skip_ok, np.concatenate(([ninf, ninf], v[:-2]))[:SS], ninf).astype(np.float32)
            m = np.maximum(np.maximum(stay, step), skip)
            back[t] = np.where(stay == m, 0, np.where(step == m, 1, 2))
            v = (m + lp[t, cls]).astype(np.float32)
    end = SS - 1 if (S == 0 or v[SS - 1] >= v[SS - 2]) else SS - 2
    score = v[end]
    if not (score > np.float32(0.5) * K_DEAD):
        return ninf, None
    states = np.zeros(Tb, dtype=np.int32)
    s = end
    for t in range(Tb - 1, 0, -1):
        states[t] = s
        s = max(s - int(back[t, s]), 0)
    states[0] = s
    return np.float32(score), states


def align_batch(logp, targets, in_lens, tgt_lens, blank):
    """logp (B, T, C) f32, targets (B, S_max) int, in_lens (B) or None, tgt_lens (B) ->
    (score (B) f32, frame_state (B, T) i32, frame_logp (B, T) f32, label_start (B, S_max) i32, label_end (B, S_max) i32)"""
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
    for b in range(B):
        Tb = T if in_lens is None else int(min(max(int(in_lens[b]), 0), T))
        S = int(min(max(int(tgt_lens[b]), 0), S_max))
        tg = [int(min(max(int(c), 0), C - 1)) for c in targets[b, :S]]
        score[b], st = align_one(lp[b, :Tb], tg, blank)
        if st is None:
            continue
        frame_state[b, :Tb] = st
        for t in range(Tb):
            s = int(st[t])
            frame_logp[b, t] = lp[b, t, tg[s >> 1] if s & 1 else blank]
            if s & 1:
                if t == 0 or st[t - 1] != s:
                    label_start[b, s >> 1] = t
                if t == Tb - 1 or st[t + 1] != s:
                    label_end[b, s >> 1] = t + 1
    return score, frame_state, frame_logp, label_start, label_end


def collapse(states, target, blank):
    """the label sequence a state path spells: classes of the states, repeats merged, blanks dropped"""
    classes = [target[s >> 1] if s & 1 else blank for s in states]
    out = []
    prev = None
    for c in classes:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def valid_path(states, S):
    """a lattice path: starts in {0, 1}, ends in {2S-1, 2S}, moves by 0 / 1 / 2 with the skip only from an odd state to an odd one"""
    states = [int(s) for s in states]
    if not states or states[0] not in (0, 1) or states[-1] not in (2 * S, 2 * S - 1) or min(states) < 0:
        return False
    for a, b in zip(states, states[1:]):
        if b - a not in (0, 1, 2) or (b - a == 2 and not (b & 1)):
            return False
    return True


def brute_force(logp, target, blank):
    """max over every frame labelling that collapses to `target`, in f64: (best log-prob or None, number of alignments)"""
    lp = np.asarray(logp, dtype=np.float64)
    Tb, C = lp.shape
    best, n = None, 0
    for path in itertools.product(range(C), repeat=Tb):
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        if out == list(target):
            n += 1
            sc = float(sum(lp[t, c] for t, c in enumerate(path)))
            best = sc if best is None or sc > best else best
    return best, n
