"""numpy definition of CTC keyword search (include/lasr.h, lasr_ctc_kws): the oracle of csrc/ctc_kws.hip.

States j = 0 .. 2L-2 (even: label j/2, odd: the blank between two labels), emissions e_t(j) = logp[t, cls(j)] - max_c logp[t, c]
in f32, every state a pair (v, s): score and the frame its path entered state 0.  The recursion is a selection and one f32 add
of identically rounded operands, so a kernel that follows the definition agrees with this file bit for bit.  Dead states are
-inf here (the kernel's finite sentinel is reported as -inf: an end score not above -5e29 is not live)."""
import itertools

import numpy as np

NO_START = 2 ** 31 - 1      # the start of a dead state: loses every tie
DEAD_BELOW = -5e29
MAX_LABELS = 64


def search_one(lp, labels, blank):
    """lp (T, C) f32, labels: the phrase.  -> E (T,) f32 with -inf where the end state is not live, S (T,) i32 with -1 there"""
    lp = np.asarray(lp, np.float32)
    T, L = lp.shape[0], len(labels)
    assert L >= 1
    n = 2 * L - 1
    cls = np.array([labels[j // 2] if j % 2 == 0 else blank for j in range(n)], np.int64)
    skip_ok = np.array([j % 2 == 0 and j >= 2 and labels[j // 2] != labels[j // 2 - 1] for j in range(n)], bool)
    v = np.full(n, -np.inf, np.float32)
    s = np.full(n, NO_START, np.int64)
    E = np.full(T, -np.inf, np.float32)
    S = np.full(T, -1, np.int32)

    def better(av, as_, bv, bs):                    # a unless b is better: the larger v, on equal v the smaller s
        take = (bv > av) | ((bv == av) & (bs < as_))
        return np.where(take, bv, av), np.where(take, bs, as_)

    with np.errstate(invalid="ignore"):
        for t in range(T):
            m = lp[t].max()
            e = (lp[t, cls] - m).astype(np.float32)                       # one f32 subtraction
            bv, bs = v.copy(), s.copy()                                   # stay
            pv = np.concatenate([np.float32([-np.inf]), v[:-1]])
            ps = np.concatenate([[NO_START], s[:-1]])
            bv, bs = better(bv, bs, pv, ps)                               # step
            qv = np.concatenate([np.float32([-np.inf, -np.inf]), v[:-2]])[:n]
            qs = np.concatenate([[NO_START, NO_START], s[:-2]])[:n]
            qv = np.where(skip_ok, qv, np.float32(-np.inf))
            bv, bs = better(bv, bs, qv, np.where(skip_ok, qs, NO_START))  # skip
            fv = np.full(n, -np.inf, np.float32)
            fv[0] = 0.0
            bv, bs = better(bv, bs, fv, np.full(n, t, np.int64))          # fresh, state 0 only
            v = (bv.astype(np.float32) + e).astype(np.float32)            # one f32 add
            s = bs
            if v[n - 1] > DEAD_BELOW:
                E[t], S[t] = v[n - 1], s[n - 1]
    return E, S


def pick(E, S, thr, max_hits):
    """the hits of one end trace: (n_hits, spans (max_hits, 2) i32, scores (max_hits,) f32); thr an f32"""
    spans = np.full((max_hits, 2), -1, np.int32)
    scores = np.zeros(max_hits, np.float32)
    n = 0
    pending = None

    def emit(p, n):
        if n < max_hits:
            spans[n] = (p[0], p[1])
            scores[n] = p[2]
        return n + 1

    thr = np.float32(thr)
    for t in range(len(E)):
        if not E[t] >= thr:
            continue
        cand = (int(S[t]), t + 1, np.float32(E[t]))
        if pending is not None and cand[0] < pending[1]:
            if cand[2] >= pending[2]:
                pending = cand
        else:
            if pending is not None:
                n = emit(pending, n)
            pending = cand
    if pending is not None:
        n = emit(pending, n)
    return n, spans, scores


def best_of(E, S):
    """(best score, (start, end)): max_t E_t, the latest t on ties; (-inf, (-1, -1)) without a live end frame"""
    best, span = np.float32(-np.inf), (-1, -1)
    for t in range(len(E)):
        if E[t] > DEAD_BELOW and E[t] >= best:
            best, span = np.float32(E[t]), (int(S[t]), t + 1)
    return best, span


def search_batch(lp, in_lens, blank, kw_labels, kw_offsets, L_max, threshold, max_hits):
    """lasr_ctc_kws on the host, with the device's clamps: lengths into [0, T]; a phrase's start into [0, total - 1], its length
    into [1, min(L_max, labels left)], its labels into [0, C - 1].  -> (n_hits (B, K) i32, hit_span (B, K, max_hits, 2) i32,
    hit_score (B, K, max_hits) f32, best_score (B, K) f32, best_span (B, K, 2) i32)"""
    lp = np.asarray(lp, np.float32)
    B, T, C = lp.shape
    kw_labels = np.asarray(kw_labels, np.int64)
    kw_offsets = np.asarray(kw_offsets, np.int64)
    K = len(kw_offsets) - 1
    assert 1 <= L_max <= MAX_LABELS and K >= 1 and max_hits >= 1 and -1e6 < threshold <= 0
    total = int(kw_offsets[K])
    n_hits = np.zeros((B, K), np.int32)
    hit_span = np.full((B, K, max_hits, 2), -1, np.int32)
    hit_score = np.zeros((B, K, max_hits), np.float32)
    best_score = np.full((B, K), -np.inf, np.float32)
    best_span = np.full((B, K, 2), -1, np.int32)
    cache = {}
    for b in range(B):
        Tb = T if in_lens is None else min(max(int(in_lens[b]), 0), T)
        for k in range(K):
            off = int(kw_offsets[k])
            base = min(max(off, 0), max(total - 1, 0))
            L = min(max(int(kw_offsets[k + 1]) - off, 1), min(L_max, max(total - base, 1)))
            labels = tuple(int(min(max(c, 0), C - 1)) for c in kw_labels[base:base + L])
            if (b, labels) not in cache:                 # duplicate phrases: one walk
                cache[(b, labels)] = search_one(lp[b, :Tb], labels, blank)
            E, S = cache[(b, labels)]
            thr = np.float32(threshold) * np.float32(L)
            n_hits[b, k], hit_span[b, k], hit_score[b, k] = pick(E, S, thr, max_hits)
            best_score[b, k], best_span[b, k] = best_of(E, S)
    return n_hits, hit_span, hit_score, best_score, best_span


def collapse(classes, blank):
    out, prev = [], None
    for c in classes:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def brute_force(lp, labels, blank):
    """exhaustive enumeration, f64: for every end frame b, over every window [a, b] and every frame labelling of it that starts
    in l_0, ends in l_{L-1} and collapses to the phrase, the best sum of e_t and the smallest start among the labellings that
    attain it.  -> E (T,) f64 (-inf: none), S (T,) int (-1: none)"""
    lp = np.asarray(lp, np.float64)
    T, C = lp.shape
    e = lp - lp.max(axis=1, keepdims=True) if T else lp
    labels = list(labels)
    alphabet = sorted(set(labels) | {blank})
    E = np.full(T, -np.inf)
    S = np.full(T, -1, np.int64)
    for b in range(T):
        for a in range(b, -1, -1):                       # a descending: an equal score at a smaller start replaces
            n = b - a + 1
            for seq in itertools.product(alphabet, repeat=n):
                if seq[0] != labels[0] or seq[-1] != labels[-1] or collapse(seq, blank) != labels:
                    continue
                score = sum(e[a + i, c] for i, c in enumerate(seq))
                if score > -np.inf and score >= E[b]:
                    E[b], S[b] = score, a
    return E, S
