"""Seeded inputs for the word-level LM beam search tests and tools/beam_wlm_time.py: word lists, and log-probs that are peaky
around an alignment of a sentence of those words - random hot classes (test_gpu_ctc_beam_lm.peaky) would leave the lexicon
nothing to accept.

``sentence_logp``: per utterance a sentence drawn from arpa_synth.sentences(words, ...) is spelled over the vocabulary (letters,
one space between words), each label held for one to three frames, a blank frame between doubled letters (and, with p_blank,
elsewhere), the rest of the T frames blank; a sentence longer than T frames is cut, possibly inside a word.  A share of the
frames (`corrupt`) gets a random hot class instead.  The hot class gets `hot` added to N(0, sd) logits before the log-softmax."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

import arpa_synth as S


def random_words(n: int, letters: Sequence[str], seed: int, min_len: int = 1, max_len: int = 9) -> List[str]:
    """n distinct seeded random words over `letters`, short ones first exhausted: many share prefixes"""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        k = int(rng.integers(min_len, max_len + 1))
        w = "".join(letters[int(i)] for i in rng.integers(0, len(letters), k))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def alignment(labels: Sequence[int], T: int, blank: int, rng, p_blank: float = 0.3) -> List[int]:
    hot: List[int] = []
    prev = None
    for c in labels:
        if c == prev or rng.random() < p_blank:
            hot.append(blank)
        hot += [c] * int(rng.integers(1, 4))
        prev = c
    hot = hot[:T]
    return hot + [blank] * (T - len(hot))


def sentence_logp(vocab: Sequence[str], words: Sequence[str], B: int, T: int, seed: int, hot: float = 8.0, sd: float = 2.0,
                  corrupt: float = 0.1, n_words=(2, 12)):
    """(log-probs (B, T, len(vocab) + 1) f32, the sentences)"""
    C = len(vocab) + 1
    ids = {s: i for i, s in enumerate(vocab)}
    rng = np.random.default_rng(seed)
    sents = S.sentences(list(words), B, seed, n_words[0], n_words[1])
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g) * sd
    hotc = np.zeros((B, T), dtype=np.int64)
    for b, sent in enumerate(sents):
        hotc[b] = alignment([ids[ch] for ch in " ".join(sent)], T, C - 1, rng)
        bad = rng.random(T) < corrupt
        hotc[b, bad] = rng.integers(0, C, int(bad.sum()))
    x.scatter_add_(2, torch.from_numpy(hotc).unsqueeze(-1), torch.full((B, T, 1), float(hot)))
    return torch.log_softmax(x, -1), sents
