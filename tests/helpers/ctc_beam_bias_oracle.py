"""f64 oracle of the hotword-biased CTC prefix beam search (lasr_ctc_beam_decode_bias / lasr_ctc_beam_decode_lm_bias;
include/lasr.h and DESIGN.md "Beam search with hotword biasing" state the contract).

``Bank`` restates the biasing automaton over label tuples, with dictionaries instead of an image: nodes are the prefixes of
the phrases, numbered in the order the phrases first reach them (the builder's numbering, so that states compare), credit =
depth * wmax evaluated in f64 and rounded to f32 as the image stores it, everything after that in f64.  bonus / final / state
of a prefix are computed from the whole prefix (memoised per prefix), never carried along a search, so the oracle shares no
bookkeeping with the kernels.  ``Bank.count`` counts each kind of step the walks took.

``beam_search`` is ctc_beam_oracle's search (pruning, log_b / log_nb, merging, tie-break) ranked by score + bonus(prefix), and
with ``lm=(vocab, ArpaOracle, alpha, beta)`` ctc_beam_lm_oracle's: the emission terms, the early cutoff with the max_credit
slack, approx_ctc.  At the end of the utterance each entry's bonus becomes final(prefix) and the entries are re-ranked, ties by
their earlier order.  ``margin`` is those oracles' (selection boundary, cutoff_prob run, early-cutoff comparisons that matter),
extended with the gaps between neighbours of the final re-rank down to the entry after the last returned one."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import ctc_beam_lm_oracle as LO
import ctc_beam_oracle as O

NEG_INF = -math.inf
_lae, _rel = O._lae, O._rel
KINDS = ("child", "fail_suffix", "fail_root", "leaf_reset", "give_back_keep", "final_give_back")


class Bank:
    def __init__(self, phrases: Sequence[Sequence[int]], weights):
        phrases = [tuple(int(c) for c in p) for p in phrases]
        if isinstance(weights, (int, float)):
            weights = [float(weights)] * len(phrases)
        self.phrases, self.weights = phrases, [float(w) for w in weights]
        self.ids: Dict[tuple, int] = {(): 0}
        wmax: Dict[tuple, float] = {(): 0.0}
        self.end = set()
        for p, w in zip(phrases, self.weights):
            for n in range(1, len(p) + 1):
                s = p[:n]
                if s not in self.ids:
                    self.ids[s] = len(self.ids)
                wmax[s] = max(wmax.get(s, 0.0), w)
            self.end.add(p)
        self.credit = {s: float(np.float32(len(s) * wmax[s])) for s in self.ids}
        self.has_child = {s[:-1] for s in self.ids if s}
        self.max_credit = max(self.credit.values())
        self.count = {k: 0 for k in KINDS}
        # the three definitions below, evaluated once per node: a search takes some 10^5 steps
        self._keep = {s: self.keep(s) for s in self.ids}
        self._fail = {s: self.fail(s) for s in self.ids}
        self._leaf = {s for s in self.ids if self.leaf(s)}
        self._memo: Dict[tuple, Tuple[float, tuple]] = {(): (0.0, ())}

    @property
    def n_nodes(self) -> int:
        return len(self.ids)

    def leaf(self, s: tuple) -> bool:
        return s in self.end and s not in self.has_child

    def keep(self, s: tuple) -> float:
        for n in range(len(s), 0, -1):
            if s[:n] in self.end:
                return self.credit[s[:n]]
        return 0.0

    def fail(self, s: tuple) -> tuple:
        for n in range(1, len(s)):
            if s[n:] in self.ids:
                return s[n:]
        return ()

    def step(self, v: tuple, c: int, count: bool = True) -> Tuple[tuple, float]:
        ids, fail = self.ids, self._fail
        u = v + (c,)
        if u in ids:
            delta = self.credit[u] - self.credit[v]
            kind = "child"
        else:
            w = fail[v]
            while w != () and w + (c,) not in ids:
                w = fail[w]
            u = w + (c,) if w + (c,) in ids else ()
            delta = self._keep[v] - self.credit[v] + self.credit[u]
            kind = None if v == () else "fail_suffix" if w != () else "fail_root"
            if count and v != () and self._keep[v] > 0:
                self.count["give_back_keep"] += 1
        if count and kind:
            self.count[kind] += 1
        if u in self._leaf:
            if count:
                self.count["leaf_reset"] += 1
            return (), delta
        return u, delta

    def walk(self, prefix: Sequence[int]) -> Tuple[float, tuple]:
        """(bonus, state) of the whole prefix, from the root"""
        if type(prefix) is not tuple:
            prefix = tuple(prefix)
        hit = self._memo.get(prefix)
        if hit is not None:
            return hit
        n = len(prefix) - 1                       # the longest memoised proper prefix, then the rest label by label
        while prefix[:n] not in self._memo:
            n -= 1
        b, v = self._memo[prefix[:n]]
        for i in range(n, len(prefix)):
            v, d = self.step(v, prefix[i])
            b += d
            self._memo[prefix[:i + 1]] = (b, v)
        return b, v

    def bonus(self, prefix) -> float:
        return self.walk(prefix)[0]

    def state(self, prefix) -> int:
        return self.ids[self.walk(prefix)[1]]

    def final(self, prefix, count: bool = True) -> float:
        b, v = self.walk(prefix)
        gb = self._keep[v] - self.credit[v]
        if count and v != () and gb != 0.0:
            self.count["final_give_back"] += 1
        return b + gb


def brute_bonus(phrases, weights, prefix) -> Tuple[float, float]:
    """(bonus, final) by the definition read as text: no node table, no memo; every quantity found by scanning the phrases"""
    phrases = [tuple(p) for p in phrases]
    is_node = lambda s: any(p[:len(s)] == s for p in phrases) if s else True            # noqa: E731
    credit = lambda s: float(np.float32(len(s) * max(w for p, w in zip(phrases, weights) if p[:len(s)] == s))) if s else 0.0  # noqa: E731
    is_end = lambda s: s in phrases                                                     # noqa: E731
    has_child = lambda s: any(len(p) > len(s) and p[:len(s)] == s for p in phrases)     # noqa: E731

    def keep(s):
        ends = [s[:n] for n in range(1, len(s) + 1) if is_end(s[:n])]
        return credit(ends[-1]) if ends else 0.0

    v, total = (), 0.0
    for c in prefix:
        if is_node(v + (c,)):
            u = v + (c,)
            total += credit(u) - credit(v)
        else:
            sfx = [v[n:] + (c,) for n in range(1, len(v) + 1) if is_node(v[n:] + (c,))]   # longest suffix of v first
            u = sfx[0] if sfx else ()
            total += keep(v) - credit(v) + credit(u)
        v = () if (is_end(u) and not has_child(u)) else u
    return total, total + keep(v) - credit(v)


def beam_search(logp: np.ndarray, length: int, blank: int, bank: Bank, beam_width: int, cutoff_top_n: int = 40,
                cutoff_prob: float = 1.0, n_best: int = 1, lm=None, use_filter: bool = True, stop_below: float = 0.0):
    """logp (T, C) -> ([(tokens, score, am_score, final bonus)] up to n_best, margin, early-cutoff drops).  lm: None, or
    (vocab, LO.ArpaOracle, alpha, beta); am_score is then approx_ctc, else the acoustic score.  stop_below: a caller that
    only takes inputs whose margin reaches this value gets (None, margin, drops) as soon as a frame falls short of it - the
    margin only shrinks, so the rest of the utterance cannot change that verdict."""
    lp = np.asarray(logp, dtype=np.float64)
    if lm is not None:
        vocab, arpa, alpha, beta = lm
        words = lambda p: [vocab[c] if c < len(vocab) else None for c in p]   # noqa: E731
        term_cache: Dict[tuple, float] = {}

        def term(pc):
            t = term_cache.get(pc)
            if t is None:
                t = term_cache[pc] = alpha * arpa.emission(words(pc)) + beta
            return t
    else:
        beta = 0.0
        term = lambda pc: 0.0                                                  # noqa: E731
    tot = lambda p, b, nb: _lae(b, nb) + bank.bonus(p)                         # noqa: E731  what the beam is ranked by

    beam: List[Tuple[tuple, float, float]] = [((), 0.0, NEG_INF)]              # b / nb: acoustic (+ the LM's terms), no bias
    margin, fired = math.inf, 0
    for t in range(int(length)):
        row = lp[t]
        kept, m = O.prune(row, cutoff_top_n, cutoff_prob)
        margin = min(margin, m)
        live = {p: r for r, (p, _, _) in enumerate(beam)}
        full = lm is not None and use_filter and len(beam) == beam_width
        min_cutoff = tot(*beam[-1]) + float(row[blank]) - max(0.0, beta) - bank.max_credit if full else NEG_INF
        nxt = {}

        def add(pfx, key, b=NEG_INF, nb=NEG_INF):
            if pfx in live:
                key = (live[pfx], 0, -1)
            e = nxt.get(pfx)
            if e is None:
                e = nxt[pfx] = [NEG_INF, NEG_INF, key]
            e[0] = _lae(e[0], b)
            e[1] = _lae(e[1], nb)

        near = []
        kept_lc = [(c, float(row[c])) for c in kept]
        for r, (p, b, nb) in enumerate(beam):
            s = _lae(b, nb)
            st = s + bank.bonus(p)
            last = p[-1] if p else None
            for c, lc in kept_lc:
                if full and c != blank:
                    gap = abs(_rel(st + lc, min_cutoff))
                    if gap < LO.NEAR:
                        pc = p + (c,)
                        if c == last:
                            near.append((gap, [(p, lc + nb + bank.bonus(p)), (pc, lc + b + term(pc) + bank.bonus(pc))]))
                        else:
                            near.append((gap, [(pc, lc + s + term(pc) + bank.bonus(pc))]))
                    if st + lc < min_cutoff:
                        fired += 1
                        continue
                if c == blank:
                    add(p, (r, 0, -1), b=lc + s)
                elif c == last:
                    add(p, (r, 0, -1), nb=lc + nb)
                    add(p + (c,), (r, 1, c), nb=lc + b + term(p + (c,)))
                else:
                    add(p + (c,), (r, 1, c), nb=lc + s + term(p + (c,)))
        items = []
        for pfx, (b, nb, key) in nxt.items():
            if _lae(b, nb) != NEG_INF:
                items.append((tot(pfx, b, nb), key, pfx, b, nb))
        items.sort(key=lambda x: (-x[0], x[1]))
        bound = items[beam_width - 1][0] if len(items) >= beam_width else NEG_INF
        for gap, contribs in near:
            for pfx, v in contribs:
                e = nxt.get(pfx)
                sc = tot(pfx, e[0], e[1]) if e is not None else NEG_INF
                if v > sc + math.log(LO.EFFECT * max(1.0, abs(sc))) and \
                        max(sc, v) > bound + math.log(LO.EFFECT * max(1.0, abs(bound))):
                    margin = min(margin, gap)
        if len(items) > beam_width:
            margin = min(margin, _rel(items[beam_width - 1][0], items[beam_width][0]))
        beam = [(x[2], x[3], x[4]) for x in items[:beam_width]]
        if margin < stop_below:
            return None, margin, fired
    # end of utterance: bonus -> final, stable re-rank
    head = []
    for r, (p, b, nb) in enumerate(beam):
        s = _lae(b, nb)
        fb = bank.final(p)
        am = s - len(p) * beta - alpha * arpa.sentence(words(p)) if lm is not None else s
        head.append((s + fb, r, p, am, fb))
    head.sort(key=lambda x: (-x[0], x[1]))
    for a, b_ in zip(head[:n_best], head[1:n_best + 1]):
        margin = min(margin, _rel(a[0], b_[0]))
    out = [(x[2], x[0], x[3], x[4]) for x in head[:n_best]]
    return out, margin, fired


def beam_search_batch(logp: np.ndarray, lens: Optional[Sequence[int]], blank: int, bank: Bank, beam_width: int,
                      cutoff_top_n: int = 40, cutoff_prob: float = 1.0, n_best: int = 1, lm=None, use_filter: bool = True,
                      stop_below: float = 0.0):
    """logp (B, T, C) -> ([[(tokens, score, am_score, final bonus)] per utterance], smallest margin, early-cutoff drops);
    (None, margin, drops) from the first utterance whose margin falls below stop_below"""
    lp = np.asarray(logp, dtype=np.float64)
    B, T = lp.shape[0], lp.shape[1]
    res, margin, fired = [], math.inf, 0
    for b in range(B):
        L = T if lens is None else min(int(lens[b]), T)
        hyps, m, f = beam_search(lp[b], L, blank, bank, beam_width, cutoff_top_n, cutoff_prob, n_best, lm, use_filter, stop_below)
        margin = min(margin, m)
        fired += f
        if hyps is None:
            return None, margin, fired
        res.append(hyps)
    return res, margin, fired
