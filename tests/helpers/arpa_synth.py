"""Seeded synthetic ARPA files for the LM-fused beam search tests and tools/beam_lm_time.py.

A token stream of sentences is drawn from a sticky random Markov chain over `labels`; every n-gram of orders 1..N of the
<s>-/</s>-padded sentences is counted and given an absolute-discounting backoff estimate (log10 p = log10((count - D) / count(
context)), log10 bow(context) = log10(D * distinct continuations / count(context))).  Counting every n-gram of the stream makes
the file suffix-closed, as KenLM's lmplz output is.  <s> gets KenLM's -99 unigram log-probability.

Knobs: order 1..6 (or above, for the reject test), labels kept out of the stream (`missing`: they become OOV), no <s> anywhere
(`no_bos`), an extra multi-character word (`multichar`: a word-level LM), and a dropped lower-order n-gram whose extension stays
(`suffix_incomplete`)."""
from __future__ import annotations

import math
from collections import Counter, defaultdict
from typing import Iterable, Sequence

import numpy as np

D = 0.5


def sentences(labels: Sequence[str], n_sent: int, seed: int, min_len: int = 2, max_len: int = 12):
    rng = np.random.default_rng(seed)
    V = len(labels)
    nxt = rng.integers(0, V, size=(V, 3))          # each label prefers 3 successors
    out = []
    for _ in range(n_sent):
        k = int(rng.integers(min_len, max_len + 1))
        c = int(rng.integers(0, V))
        s = [c]
        for _ in range(k - 1):
            c = int(nxt[c, rng.integers(0, 3)]) if rng.random() < 0.7 else int(rng.integers(0, V))
            s.append(c)
        out.append([labels[i] for i in s])
    return out


def arpa_text(sents: Iterable[Sequence[str]], order: int, no_bos: bool = False, multichar: bool = False,
              suffix_incomplete: bool = False) -> str:
    counts = [Counter() for _ in range(order + 1)]
    for s in sents:
        padded = ["<s>"] + list(s) + ["</s>"]
        for n in range(1, order + 1):
            for i in range(len(padded) - n + 1):
                g = tuple(padded[i:i + n])
                if n == 1 and g == ("<s>",):
                    continue
                counts[n][g] += 1
    counts[1][("<s>",)] = sum(1 for _ in counts[2]) if order >= 2 else 1
    if multichar:
        counts[1][("ab",)] = 1
    ctx_total, ctx_types = defaultdict(int), defaultdict(int)
    for n in range(2, order + 1):
        for g, c in counts[n].items():
            ctx_total[g[:-1]] += c
            ctx_types[g[:-1]] += 1
    total1 = sum(c for g, c in counts[1].items() if g != ("<s>",))
    sections = []
    for n in range(1, order + 1):
        lines = []
        for g in sorted(counts[n]):
            if no_bos and "<s>" in g:
                continue
            c = counts[n][g]
            if n == 1:
                lp = -99.0 if g == ("<s>",) else math.log10(max(c - D, 0.1) / total1)
            else:
                lp = math.log10((c - D) / ctx_total[g[:-1]])
            line = "%.6f\t%s" % (lp, " ".join(g))
            if n < order and g in ctx_total:
                line += "\t%.6f" % math.log10(D * ctx_types[g] / ctx_total[g])
            elif n < order:
                line += "\t0"
            lines.append(line)
        sections.append(lines)
    if suffix_incomplete and order >= 3:
        # drop a 2-gram that is the suffix of a stored 3-gram
        tri = next(g for g in sorted(counts[3]) if "<s>" not in g)
        drop = "\t%s\t" % " ".join(tri[1:])
        sections[1] = [ln for ln in sections[1] if drop not in ln + "\t"]
    out = ["\\data\\"] + ["ngram %d=%d" % (n + 1, len(sec)) for n, sec in enumerate(sections)] + [""]
    for n, sec in enumerate(sections):
        out += ["\\%d-grams:" % (n + 1)] + sec + [""]
    out.append("\\end\\")
    return "\n".join(out) + "\n"


def write_arpa(path, labels: Sequence[str], order: int, n_sent: int = 300, seed: int = 0, missing: Sequence[str] = (),
               no_bos: bool = False, multichar: bool = False, suffix_incomplete: bool = False, max_len: int = 12) -> str:
    """write a synthetic ARPA LM over `labels` minus `missing` to `path`; returns the path as a string"""
    keep = [w for w in labels if w not in set(missing) and w.strip() == w and w]     # a blank label cannot be an ARPA word
    text = arpa_text(sentences(keep, n_sent, seed, max_len=max_len), order, no_bos, multichar, suffix_incomplete)
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    return str(path)
