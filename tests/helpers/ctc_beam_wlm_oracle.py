"""f64 oracle of the CTC prefix beam search fused with a word-level n-gram LM and its lexicon, which lasr_ctc_beam_decode_wlm
implements (include/lasr.h, DESIGN.md "Beam search with a word-level LM").

On top of ctc_beam_oracle's search (pruning, log_b / log_nb, merging, tie-break) and ctc_beam_lm_oracle's early cutoff:
- the lexicon is a dict trie over the label ids of the spellable LM words (every code point a one-code-point, non-space label);
  a prefix sits at the node its letters since the last space lead to; p + c (c neither space nor blank) exists only where that
  node has a child c, p + space only where the node is a complete word; what does not exist contributes nothing;
- a non-space label adds no term; the space after word w adds alpha * lm(w | previous N-1 words, <s>-padded) + beta, with
  ArpaOracle used as a word LM;
- at the end a non-empty prefix that does not end in the space gets alpha * lm(w | ...) + beta if its node is a complete word,
  alpha * OOV_SCORE + beta if not; the final entries are then re-ranked by the new fused score, ties by their earlier order;
- the acoustic score is the fused score minus every term added.

``margin`` is ctc_beam_lm_oracle's, extended with the gaps between neighbours of the final re-rank down to the entry after the
last returned one.  Lexicon decisions are exact integer facts and need no margin."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import ctc_beam_lm_oracle as LO
import ctc_beam_oracle as O

NEG_INF = -math.inf
OOV_SCORE = LO.OOV_SCORE
_lae, _rel = O._lae, O._rel
NEAR, EFFECT = LO.NEAR, LO.EFFECT
WORD = "$"                   # trie key of a node's word (label ids are ints, so it cannot clash)


def spell(word: str, vocab: Sequence[str], space: int) -> Optional[List[int]]:
    """the label ids of `word`, or None where some code point is no one-code-point, non-space label"""
    ids = {}
    for i, s in enumerate(vocab):
        if i != space and len(s) == 1:
            ids.setdefault(s, i)
    out = [ids.get(ch) for ch in word]
    return None if (not out or any(c is None for c in out)) else out


def build_trie(lm_words: Sequence[str], vocab: Sequence[str], space: int):
    """(trie, spellable words, dropped words) over the LM's words but <s>, </s>, <unk>; a node is a dict label id -> node, with
    node[WORD] the word where it is complete"""
    root: dict = {}
    kept, dropped = [], []
    for w in lm_words:
        if w in ("<s>", "</s>", "<unk>"):
            continue
        ids = spell(w, vocab, space)
        if ids is None:
            dropped.append(w)
            continue
        node = root
        for c in ids:
            node = node.setdefault(c, {})
        node[WORD] = w
        kept.append(w)
    return root, kept, dropped


class WordLm:
    """an ArpaOracle used as a word LM, with the lexicon of `vocab`"""

    def __init__(self, lm: LO.ArpaOracle, vocab: Sequence[str]):
        assert list(vocab).count(" ") == 1
        self.lm, self.vocab, self.space = lm, list(vocab), list(vocab).index(" ")
        words = sorted(w[0] for w in lm.ngrams if len(w) == 1)
        self.trie, self.words, self.dropped = build_trie(words, self.vocab, self.space)

    @classmethod
    def from_file(cls, path, vocab) -> "WordLm":
        return cls(LO.ArpaOracle.from_file(path), vocab)

    def state(self, prefix: Sequence[int]):
        """(finished words, node of the unfinished word or None when the prefix left the lexicon)"""
        words, node = [], self.trie
        for c in prefix:
            if node is None:
                return words, None
            if c == self.space:
                if WORD not in node:
                    return words, None
                words.append(node[WORD])
                node = self.trie
            else:
                node = node.get(c)
        return words, node

    def exists(self, prefix: Sequence[int]) -> bool:
        return self.state(prefix)[1] is not None

    def word_term(self, words: Sequence[str], alpha: float, beta: float) -> float:
        return alpha * self.lm.emission(list(words)) + beta

    def bonus(self, prefix: Sequence[int], alpha: float, beta: float) -> float:
        """the sum of the terms of the prefix's spaces"""
        words, _ = self.state(prefix)
        return sum(self.word_term(words[:i + 1], alpha, beta) for i in range(len(words)))

    def end_term(self, prefix: Sequence[int], alpha: float, beta: float) -> float:
        if not prefix or prefix[-1] == self.space:
            return 0.0
        words, node = self.state(prefix)
        if WORD in node:
            return self.word_term(words + [node[WORD]], alpha, beta)
        return alpha * OOV_SCORE + beta


def beam_search(logp: np.ndarray, length: int, blank: int, wl: WordLm, alpha: float, beta: float, beam_width: int,
                cutoff_top_n: int = 40, cutoff_prob: float = 1.0, n_best: int = 1, use_filter: bool = True, end_term: bool = True):
    """logp (T, C) -> ([(tokens, fused, acoustic)] up to n_best, margin, early-cutoff drops, lexicon rejections, reranked)"""
    lp = np.asarray(logp, dtype=np.float64)
    space = wl.space
    info: Dict[tuple, Tuple[bool, float]] = {(): (True, 0.0)}      # prefix -> (exists, bonus)

    def look(pc):
        r = info.get(pc)
        if r is None:
            ok = wl.exists(pc)
            r = info[pc] = (ok, wl.bonus(pc, alpha, beta) if ok else 0.0)
        return r

    def term(pc):             # what the last label of pc added (0 unless it is the space)
        return look(pc)[1] - look(pc[:-1])[1]

    beam: List[Tuple[tuple, float, float]] = [((), 0.0, NEG_INF)]
    margin, fired, rejected = math.inf, 0, 0
    for t in range(int(length)):
        row = lp[t]
        kept, m = O.prune(row, cutoff_top_n, cutoff_prob)
        margin = min(margin, m)
        live = {p: r for r, (p, _, _) in enumerate(beam)}
        full = use_filter and len(beam) == beam_width
        min_cutoff = _lae(beam[-1][1], beam[-1][2]) + float(row[blank]) - max(0.0, beta) if full else NEG_INF
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
        for r, (p, b, nb) in enumerate(beam):
            s = _lae(b, nb)
            last = p[-1] if p else None
            for c in kept:
                lc = float(row[c])
                pc = p + (c,)
                ext = c != blank and look(pc)[0]          # the extension p -> p + c exists in the lexicon
                if c != blank and not ext:
                    rejected += 1
                if full and c != blank:
                    gap = abs(_rel(s + lc, min_cutoff))
                    if gap < NEAR:
                        contribs = []
                        if c == last:
                            contribs.append((p, lc + nb))
                            if ext:
                                contribs.append((pc, lc + b + term(pc)))
                        elif ext:
                            contribs.append((pc, lc + s + term(pc)))
                        if contribs:
                            near.append((gap, contribs))
                    if s + lc < min_cutoff:
                        fired += 1
                        continue
                if c == blank:
                    add(p, (r, 0, -1), b=lc + s)
                elif c == last:
                    add(p, (r, 0, -1), nb=lc + nb)
                    if ext:
                        add(pc, (r, 1, c), nb=lc + b + term(pc))
                elif ext:
                    add(pc, (r, 1, c), nb=lc + s + term(pc))
        items = []
        for pfx, (b, nb, key) in nxt.items():
            sc = _lae(b, nb)
            if sc != NEG_INF:
                items.append((sc, key, pfx, b, nb))
        items.sort(key=lambda x: (-x[0], x[1]))
        bound = items[beam_width - 1][0] if len(items) >= beam_width else NEG_INF
        for gap, contribs in near:
            for pfx, v in contribs:
                e = nxt.get(pfx)
                st = _lae(e[0], e[1]) if e is not None else NEG_INF
                if v > st + math.log(EFFECT * max(1.0, abs(st))) and \
                        max(st, v) > bound + math.log(EFFECT * max(1.0, abs(bound))):
                    margin = min(margin, gap)
        if len(items) > beam_width:
            margin = min(margin, _rel(items[beam_width - 1][0], items[beam_width][0]))
        beam = [(x[2], x[3], x[4]) for x in items[:beam_width]]
    # the end-of-utterance term and the re-rank (stable: ties keep their earlier order)
    final = []
    for r, (p, b, nb) in enumerate(beam):
        fused = _lae(b, nb)
        e = wl.end_term(p, alpha, beta) if end_term else 0.0
        final.append((fused + e, r, p, fused - look(p)[1]))
    final.sort(key=lambda x: (-x[0], x[1]))
    head = final[:n_best + 1]
    reranked = [x[1] for x in head] != list(range(len(head)))      # the order before the term was 0, 1, 2, ...
    for a, b_ in zip(head, head[1:]):
        margin = min(margin, _rel(a[0], b_[0]))
    out = [(p, f, am) for f, _, p, am in final[:n_best]]
    return out, margin, fired, rejected, reranked


def beam_search_batch(logp: np.ndarray, lens: Optional[Sequence[int]], blank: int, wl: WordLm, alpha: float, beta: float,
                      beam_width: int, cutoff_top_n: int = 40, cutoff_prob: float = 1.0, n_best: int = 1, use_filter: bool = True,
                      end_term: bool = True):
    """logp (B, T, C) -> (hypotheses per utterance, smallest margin, early-cutoff drops, lexicon rejections, any reranked)"""
    lp = np.asarray(logp, dtype=np.float64)
    B, T = lp.shape[0], lp.shape[1]
    res, margin, fired, rejected, reranked = [], math.inf, 0, 0, False
    for b in range(B):
        L = T if lens is None else min(int(lens[b]), T)
        hyps, m, f, rj, rr = beam_search(lp[b], L, blank, wl, alpha, beta, beam_width, cutoff_top_n, cutoff_prob, n_best,
                                         use_filter, end_term)
        res.append(hyps)
        margin = min(margin, m)
        fired += f
        rejected += rj
        reranked = reranked or rr
    return res, margin, fired, rejected, reranked
