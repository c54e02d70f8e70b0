"""f64 oracle of the LM-fused CTC prefix beam search that lasr_ctc_beam_decode_lm implements: ctc_decoders'
ctc_beam_search_decoder with a character-based Scorer, restated (include/lasr.h, DESIGN.md "Beam search with an n-gram LM").

On top of ctc_beam_oracle's search (pruning, log_b / log_nb, merging, tie-break):
- every label emission p -> p+c adds alpha * lm(c | p) + beta (from score(p) when c != last(p), from log_b(p) when it repeats);
- lm(c | p): the last N labels of p+c (left-padded with <s>) scored by ARPA backoff, log10 -> natural log by dividing by
  NUM_FLT_LOGE; -1000 (unconverted) when any word of the n-gram is outside the LM's vocabulary;
- early cutoff: with a full beam (beam_width prefixes after the previous frame), min_cutoff = score(last prefix) + logp[blank]
  - max(0, beta), and (p, c) contributes nothing where score(p) + logp[c] < min_cutoff;
- ranking by the fused score; approx_ctc = fused - k * beta - alpha * sent_lm.

``margin`` extends ctc_beam_oracle's with the early-cutoff comparisons (blank excluded: it passes by construction) whose
outcome matters: deciding the other way would move the entry it feeds by more than EFFECT (relative; log(1 + e^d) <= e^d),
for an entry that is, or could become, part of the beam.  The other comparisons (~10^5 per utterance) could go either way
and move no score by more than the tolerance the tests hold f32 results to, nor cross a selection boundary, which the margin
keeps further apart."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import ctc_beam_oracle as O

NUM_FLT_LOGE = 0.4342944819
OOV_SCORE = -1000.0
NEG_INF = -math.inf
_lae, _rel = O._lae, O._rel
NEAR = 1e-3            # early-cutoff comparisons closer than this (relative) are checked for their effect
EFFECT = 1e-6          # a flip that moves no score by more than this (relative) cannot change an f32 result's choices


class ArpaOracle:
    """a text ARPA model as a dict of n-gram tuples -> (log10 p, log10 bow)"""

    def __init__(self, text: str):
        self.ngrams: Dict[tuple, Tuple[float, float]] = {}
        self.order = 0
        sec = 0
        for raw in text.splitlines():
            line = raw.strip()
            if not line:
                continue
            if line.startswith("\\"):
                if line.endswith("-grams:"):
                    sec = int(line[1:-7])
                    self.order = max(self.order, sec)
                elif line == "\\end\\":
                    break
                continue
            if sec == 0:
                continue
            tok = line.split()
            lp = float(tok[0])
            words = tuple(tok[1:1 + sec])
            bow = float(tok[1 + sec]) if len(tok) == sec + 2 else 0.0
            self.ngrams[words] = (lp, bow)
        self.vocab = {w[0] for w in self.ngrams if len(w) == 1 and w[0] != "<unk>"}

    @classmethod
    def from_file(cls, path) -> "ArpaOracle":
        with open(path, encoding="utf-8") as f:
            return cls(f.read())

    def cond_log10(self, ngram: Sequence[str]) -> float:
        """textbook backoff: log10 p of the longest stored suffix, plus the backoffs of the longer contexts"""
        ctx, c = tuple(ngram[:-1]), ngram[-1]
        n = len(ctx)
        m = n
        while m >= 0:
            key = ctx[n - m:] + (c,)
            if key in self.ngrams:
                break
            m -= 1
        lp = self.ngrams[ctx[n - m:] + (c,)][0]
        bo = sum(self.ngrams.get(ctx[n - j:], (0.0, 0.0))[1] for j in range(m + 1, n + 1))
        return lp + bo

    def score(self, ngram: Sequence[Optional[str]]) -> float:
        """natural-log lm of the last word of an N-word n-gram (None = a label with no string)"""
        if any(w is None or w not in self.vocab for w in ngram):
            return OOV_SCORE
        return self.cond_log10(ngram) / NUM_FLT_LOGE

    def ngram(self, words: Sequence[Optional[str]]) -> List[Optional[str]]:
        """the last N words of <s>-padded `words`"""
        N = self.order
        w = list(words)[-N:]
        return ["<s>"] * (N - len(w)) + w

    def emission(self, words: Sequence[Optional[str]]) -> float:
        return self.score(self.ngram(words))

    def sentence(self, words: Sequence[Optional[str]]) -> float:
        """ctc_decoders' get_sent_log_prob: <s>^(N-1) words </s> (<s>^N </s> for no words) over N-word windows"""
        N = self.order
        sent = (["<s>"] * N if not words else ["<s>"] * (N - 1) + list(words)) + ["</s>"]
        return sum(self.score(sent[i:i + N]) for i in range(len(sent) - N + 1))


def beam_search(logp: np.ndarray, length: int, blank: int, vocab: Sequence[str], lm: ArpaOracle, alpha: float, beta: float,
                beam_width: int, cutoff_top_n: int = 40, cutoff_prob: float = 1.0, n_best: int = 1, use_filter: bool = True):
    """logp (T, C) -> ([(tokens, fused, approx_ctc)] up to n_best, margin, number of (p, c) the early cutoff dropped)"""
    lp = np.asarray(logp, dtype=np.float64)
    words = lambda p: [vocab[c] if c < len(vocab) else None for c in p]   # noqa: E731
    term_cache: Dict[tuple, float] = {}

    def term(pc):
        t = term_cache.get(pc)
        if t is None:
            t = term_cache[pc] = alpha * lm.emission(words(pc)) + beta
        return t

    beam: List[Tuple[tuple, float, float]] = [((), 0.0, NEG_INF)]
    margin, fired = math.inf, 0
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

        near = []          # early-cutoff comparisons close to the threshold: (gap, [(target prefix, contribution)])
        for r, (p, b, nb) in enumerate(beam):
            s = _lae(b, nb)
            last = p[-1] if p else None
            for c in kept:
                lc = float(row[c])
                if full and c != blank:
                    gap = abs(_rel(s + lc, min_cutoff))
                    if gap < NEAR:
                        if c == last:
                            near.append((gap, [(p, lc + nb), (p + (c,), lc + b + term(p + (c,)))]))
                        else:
                            near.append((gap, [(p + (c,), lc + s + term(p + (c,)))]))
                    if s + lc < min_cutoff:
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
            sc = _lae(b, nb)
            if sc != NEG_INF:
                items.append((sc, key, pfx, b, nb))
        items.sort(key=lambda x: (-x[0], x[1]))
        bound = items[beam_width - 1][0] if len(items) >= beam_width else NEG_INF
        for gap, contribs in near:
            # the comparison counts where deciding it the other way could change the result beyond f32 resolution: the
            # contribution is not negligible against its target, and the target is (or could become) part of the beam
            for pfx, v in contribs:
                e = nxt.get(pfx)
                st = _lae(e[0], e[1]) if e is not None else NEG_INF
                if v > st + math.log(EFFECT * max(1.0, abs(st))) and \
                        max(st, v) > bound + math.log(EFFECT * max(1.0, abs(bound))):
                    margin = min(margin, gap)
        if len(items) > beam_width:
            margin = min(margin, _rel(items[beam_width - 1][0], items[beam_width][0]))
        beam = [(x[2], x[3], x[4]) for x in items[:beam_width]]
    out = []
    for p, b, nb in beam[:n_best]:
        fused = _lae(b, nb)
        out.append((p, fused, fused - len(p) * beta - alpha * lm.sentence(words(p))))
    return out, margin, fired


def beam_search_batch(logp: np.ndarray, lens: Optional[Sequence[int]], blank: int, vocab, lm: ArpaOracle, alpha: float,
                      beta: float, beam_width: int, cutoff_top_n: int = 40, cutoff_prob: float = 1.0, n_best: int = 1,
                      use_filter: bool = True):
    """logp (B, T, C) -> ([[(tokens, fused, approx_ctc)] per utterance], smallest margin, total early-cutoff drops)"""
    lp = np.asarray(logp, dtype=np.float64)
    B, T = lp.shape[0], lp.shape[1]
    res, margin, fired = [], math.inf, 0
    for b in range(B):
        L = T if lens is None else min(int(lens[b]), T)
        hyps, m, f = beam_search(lp[b], L, blank, vocab, lm, alpha, beta, beam_width, cutoff_top_n, cutoff_prob, n_best,
                                 use_filter)
        res.append(hyps)
        margin = min(margin, m)
        fired += f
    return res, margin, fired
