"""f64 oracle of the CTC prefix beam search that lasr_ctc_beam_decode implements (ctc_decoders' ctc_beam_search_decoder with no
external scorer; blank = C - 1 in this project).

Contract, shared with csrc/ctc_beam.hip:
- frame pruning: classes ordered by (log-prob desc, id asc); with cutoff_prob < 1 the shortest leading run whose cumulative
  exp(logp) reaches cutoff_prob, then at most cutoff_top_n of them;
- a prefix holds (log_b, log_nb), score = logaddexp(log_b, log_nb); the beam starts as {(): (0, -inf)};
- per kept class c and live prefix p (s = score(p)): blank -> next[p].b += lc + s; c == last(p) -> next[p].nb += lc + p.nb and
  next[p+c].nb += lc + p.b; otherwise next[p+c].nb += lc + s (log-add; p+c merges with a live prefix equal to it);
- the beam_width best entries of `next` with a finite score survive, ties broken by (rank of the source prefix, no new label
  before a label, label id); a p+c that merged into a live prefix keeps that prefix's key.  The beam is kept in that order.

``margin`` is the smallest relative gap, over every frame, between what was kept and the best of what was dropped: the
beam-selection boundary (score of the last survivor against the best dropped entry) and the cumulative-probability run
against cutoff_prob.  An f32 implementation can only be held to the oracle's exact choices where this margin is well above
its rounding.  The cutoff_top_n cut compares the input log-probs themselves, with the same tie-break, so it is exact in any
precision and needs no margin."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

NEG_INF = -math.inf


def _lae(a: float, b: float) -> float:
    if a == NEG_INF:
        return b
    if b == NEG_INF:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(min(a, b) - m))


def _rel(a: float, b: float) -> float:
    return (a - b) / max(1.0, abs(a))


def prune(row: np.ndarray, cutoff_top_n: int, cutoff_prob: float) -> Tuple[List[int], float]:
    """kept class ids (in (logp desc, id asc) order) of one frame, and this frame's pruning margin"""
    C = row.shape[0]
    order = np.lexsort((np.arange(C), -row))
    n = min(int(cutoff_top_n), C)
    margin = math.inf
    if cutoff_prob < 1.0:
        cum, L = 0.0, 0
        for c in order:
            cum_prev = cum
            cum += math.exp(row[c])
            L += 1
            if cum >= cutoff_prob or L >= n:
                break
        # both sums around the cut must sit clear of cutoff_prob (conservative: also where the run ended on cutoff_top_n)
        margin = min(margin, abs(cum - cutoff_prob) / cutoff_prob)
        if L > 1:
            margin = min(margin, abs(cutoff_prob - cum_prev) / cutoff_prob)
        n = L
    return [int(c) for c in order[:n]], margin


def beam_search(logp: np.ndarray, length: int, blank: int, beam_width: int, cutoff_top_n: int = 40,
                cutoff_prob: float = 1.0, n_best: int = 1):
    """logp (T, C) log-probs of one utterance -> ([(tokens tuple, score)] of up to n_best entries, margin)"""
    lp = np.asarray(logp, dtype=np.float64)
    beam: List[Tuple[tuple, float, float]] = [((), 0.0, NEG_INF)]
    margin = math.inf
    for t in range(int(length)):
        row = lp[t]
        kept, m = prune(row, cutoff_top_n, cutoff_prob)
        margin = min(margin, m)
        live = {p: r for r, (p, _, _) in enumerate(beam)}
        nxt = {}

        def add(pfx, key, b=NEG_INF, nb=NEG_INF):
            if pfx in live:
                key = (live[pfx], 0, -1)
            e = nxt.get(pfx)
            if e is None:
                e = nxt[pfx] = [NEG_INF, NEG_INF, key]
            e[0] = _lae(e[0], b)
            e[1] = _lae(e[1], nb)

        for r, (p, b, nb) in enumerate(beam):
            s = _lae(b, nb)
            last = p[-1] if p else None
            for c in kept:
                lc = float(row[c])
                if c == blank:
                    add(p, (r, 0, -1), b=lc + s)
                elif c == last:
                    add(p, (r, 0, -1), nb=lc + nb)
                    add(p + (c,), (r, 1, c), nb=lc + b)
                else:
                    add(p + (c,), (r, 1, c), nb=lc + s)
        items = []
        for pfx, (b, nb, key) in nxt.items():
            sc = _lae(b, nb)
            if sc != NEG_INF:
                items.append((sc, key, pfx, b, nb))
        items.sort(key=lambda x: (-x[0], x[1]))
        if len(items) > beam_width:
            margin = min(margin, _rel(items[beam_width - 1][0], items[beam_width][0]))
        beam = [(x[2], x[3], x[4]) for x in items[:beam_width]]
    out = [(p, _lae(b, nb)) for p, b, nb in beam[:n_best]]
    return out, margin


def beam_search_batch(logp: np.ndarray, lens: Optional[Sequence[int]], blank: int, beam_width: int, cutoff_top_n: int = 40,
                      cutoff_prob: float = 1.0, n_best: int = 1):
    """logp (B, T, C) -> ([[(tokens, score)] per utterance], smallest margin)"""
    lp = np.asarray(logp, dtype=np.float64)
    B, T = lp.shape[0], lp.shape[1]
    res, margin = [], math.inf
    for b in range(B):
        L = T if lens is None else min(int(lens[b]), T)
        hyps, m = beam_search(lp[b], L, blank, beam_width, cutoff_top_n, cutoff_prob, n_best)
        res.append(hyps)
        margin = min(margin, m)
    return res, margin


def collapse(path: Sequence[int], blank: int) -> tuple:
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return tuple(out)


def brute_force(logp: np.ndarray, blank: int) -> dict:
    """every labelling of a (T, C) utterance -> its exact log-likelihood, by enumerating all C^T paths (tiny T, C only)"""
    lp = np.asarray(logp, dtype=np.float64)
    T, C = lp.shape
    acc = {}
    for path in np.ndindex(*([C] * T)):
        s = float(sum(lp[t, c] for t, c in enumerate(path)))
        lab = collapse(path, blank)
        acc[lab] = _lae(acc.get(lab, NEG_INF), s)
    return acc
