"""``BeamSearchDecoderWithLM`` of the reference (beam_search.py:17-57) on the HIP CTC prefix beam search (csrc/ctc_beam.hip).

The reference runs ctc_decoders' ``ctc_beam_search_decoder_batch`` on the host, optionally with a KenLM scorer.  Here the
search runs on the GPU: one launch prunes every frame, one workgroup per utterance searches it.  With ``lm_path`` (a text
ARPA file) the search is fused with that LM (ops.load_arpa / ops.ctc_beam_decode_lm).  A character n-gram LM, as the
reference's ckpt/lm/readme.md trains: ``alpha`` weighs its natural-log score, ``beta`` is added per emitted label.  A word
n-gram LM, with a vocabulary that has exactly one " " label: only words the LM knows and the labels can spell are decoded,
``alpha`` weighs the LM score of each word, given at the space after it or at the end of the utterance, ``beta`` is added per
word.  KenLM binary models, and word-level LMs with a vocabulary without a space label, raise NotImplementedError.
``num_cpus`` is accepted and ignored.  The blank is the class
after the vocabulary (ctc_decoders' ``blank_id = vocabulary.size()``).

``hotwords`` (a list of ``str`` or ``(str, weight)``) biases the search, with or without a character LM, towards hypotheses that
spell those phrases (ops.build_hotwords / ops.ctc_beam_decode_biased; include/lasr.h states the scoring).  ``set_hotwords``
swaps the bank without reloading the LM; ``None`` or ``[]`` turns the biasing off."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops


def parse_hotwords(vocab: Sequence[str], hotwords, weight: float = 2.0) -> Tuple[List[List[int]], List[float]]:
    """hotwords, a list of ``str`` or ``(str, weight)``, -> (label-id lists, weights).  A phrase is mapped code point by code
    point through `vocab` (the first class of a string that occurs twice); it may contain " " where the vocabulary has that
    label.  A character outside the vocabulary raises ValueError naming the phrase and the character; so does an empty phrase.
    Needs no GPU."""
    index = {}
    for i, s in enumerate(vocab):
        index.setdefault(s, i)
    phrases, weights = [], []
    for k, item in enumerate(hotwords):
        text, w = (item, weight) if isinstance(item, str) else (item[0], item[1])
        if not isinstance(text, str):
            raise TypeError("hotword %d: expected str or (str, weight), got %r" % (k, item))
        if not text:
            raise ValueError("hotword %d is empty" % k)
        ids = []
        for ch in text:
            if ch not in index:
                raise ValueError("hotword %d (%r): character %r is not in the vocabulary" % (k, text, ch))
            ids.append(index[ch])
        phrases.append(ids)
        weights.append(float(w))
    return phrases, weights


class BeamSearchDecoderWithLM(torch.nn.Module):

    def __init__(self, vocab, beam_width, alpha, beta, lm_path, num_cpus, cutoff_prob=1.0, cutoff_top_n=40, device="cuda",
                 hotwords=None, hotword_weight: float = 2.0):
        """hotword_weight: the weight of a hotword given without one, in natural-log units per matched label.  The default 2.0
        is a starting value: nobody has tuned it on a trained model."""
        super().__init__()
        self.vocab = list(vocab)
        # a missing file raises ops.ArpaNotFoundError (FileNotFoundError and NotImplementedError) before any device work
        self.scorer = None if lm_path is None else ops.load_arpa(lm_path, self.vocab, device, alpha, beta)
        self.beam_width = int(beam_width)
        self.alpha, self.beta = alpha, beta
        self.num_cpus = num_cpus
        self.cutoff_prob = float(cutoff_prob)
        self.cutoff_top_n = int(cutoff_top_n)
        self.device = torch.device(device)
        self.hotword_weight = float(hotword_weight)
        self.hotwords: Optional[ops.HotwordBank] = None
        self.set_hotwords(hotwords)

    def set_hotwords(self, hotwords, weight: Optional[float] = None) -> None:
        """Swap the phrase bank (the LM stays loaded).  hotwords: a list of ``str`` or ``(str, weight)``; ``None`` or ``[]`` turns
        the biasing off, and the decoder makes the unbiased calls again.  weight: for phrases given without one (default: the
        decoder's hotword_weight).  A word-level LM raises NotImplementedError, a character outside the vocabulary ValueError."""
        if not hotwords:
            self.hotwords = None
            return
        if self.scorer is not None and not self.scorer.is_character_based():
            raise NotImplementedError("hotwords with a word-level LM are not implemented: its lexicon confines the search to "
                                      "the LM's words")
        phrases, weights = parse_hotwords(self.vocab, hotwords, self.hotword_weight if weight is None else float(weight))
        self.hotwords = ops.build_hotwords(phrases, weights, n_classes=len(self.vocab) + 1, blank=len(self.vocab), device=self.device)

    def search(self, log_probs, log_probs_length, n_best: int = 1):
        """(B, T, C) log-probs (numpy or tensor) + (B) lengths -> (tokens (B, n_best, T), n_tokens (B, n_best), scores (B, n_best))
        as device tensors (ops.ctc_beam_decode; with an LM the fused scores of ops.ctc_beam_decode_lm)"""
        return self.search_full(log_probs, log_probs_length, n_best)[:3]

    def search_full(self, log_probs, log_probs_length, n_best: int = 1):
        """search() plus, when an LM is fused, ctc_decoders' approx_ctc scores (B, n_best) for a character LM and the acoustic
        scores for a word LM (None without an LM).  With hotwords the first three are the biased search's and the fourth is
        its am_scores: the acoustic scores without an LM, approx_ctc with a character LM."""
        lp = torch.as_tensor(np.ascontiguousarray(log_probs)) if isinstance(log_probs, np.ndarray) else log_probs
        dev = lp.device if lp.is_cuda else self.device
        lp = lp.to(dev, torch.float32).contiguous()
        if lp.shape[-1] != len(self.vocab) + 1:
            raise ValueError("log-probs have %d classes; the vocabulary has %d labels + blank" % (lp.shape[-1], len(self.vocab)))
        lens = None
        if log_probs_length is not None:
            lens = torch.as_tensor(np.asarray(log_probs_length) if not torch.is_tensor(log_probs_length) else log_probs_length)
            lens = lens.to(dev, torch.int32).contiguous()
        if self.scorer is not None and self.scorer.image.device != lp.device:
            self.scorer.image = self.scorer.image.to(lp.device)
        if self.hotwords is not None:
            if self.hotwords.image.device != lp.device:
                self.hotwords.image = self.hotwords.image.to(lp.device)
            return ops.ctc_beam_decode_biased(lp, lens, len(self.vocab), self.hotwords, self.beam_width, self.cutoff_top_n,
                                              self.cutoff_prob, n_best, self.scorer, None if self.scorer is None else self.alpha,
                                              None if self.scorer is None else self.beta)[:4]
        if self.scorer is not None:
            return ops.ctc_beam_decode_lm(lp, lens, len(self.vocab), self.scorer, self.beam_width, self.cutoff_top_n,
                                          self.cutoff_prob, n_best, self.alpha, self.beta)
        return ops.ctc_beam_decode(lp, lens, len(self.vocab), self.beam_width, self.cutoff_top_n, self.cutoff_prob,
                                   n_best) + (None,)

    def open_stream(self, n_streams: int = 1, t_cap: int = 3000, n_best: int = 1) -> ops.CtcBeamStream:
        """A resumable search configured like this decoder (LM kind, alpha / beta, hotwords as they are now, widths and cutoffs):
        ops.CtcBeamStream, whose feed() takes the log-probs chunk by chunk and returns, after every chunk, what search_full
        returns for the frames so far.  t_cap: the most frames a stream takes between two resets.  A later set_hotwords does
        not reach a stream that is already open."""
        return ops.CtcBeamStream(n_streams, len(self.vocab) + 1, len(self.vocab), self.beam_width, self.cutoff_top_n, self.cutoff_prob,
                                 n_best, t_cap, lm=self.scorer, bank=self.hotwords,
                                 alpha=None if self.scorer is None else self.alpha,
                                 beta=None if self.scorer is None else self.beta, device=self.device)

    def _text(self, toks) -> str:
        return "".join(self.vocab[int(c)] for c in toks)

    @torch.no_grad()
    def forward(self, log_probs, log_probs_length) -> List[str]:
        """the best hypothesis of every utterance as text (beam_search.py:31-47); with an LM, the best by the fused score"""
        tokens, n, _ = self.search(log_probs, log_probs_length, 1)
        tokens, n = tokens.cpu().numpy(), n.cpu().numpy()
        return [self._text(tokens[b, 0, :max(int(n[b, 0]), 0)]) for b in range(tokens.shape[0])]

    @torch.no_grad()
    def decode_nbest(self, log_probs, log_probs_length, n_best=None) -> List[List[Tuple[float, str]]]:
        """ctc_decoders' output: per utterance [(score, text), ...], best first (up to n_best, default beam_width).  With an LM
        the list is ranked by the fused score and each score is ctc_decoders' approx_ctc (a word LM: the acoustic score).
        With hotwords the list is ranked by the biased score (search_full's third element) while each score reported here
        stays free of the bias: the acoustic log-probability without an LM, approx_ctc with a character LM.  A caller that
        wants the score the ranking used takes it from search_full."""
        n_best = self.beam_width if n_best is None else int(n_best)
        tokens, n, scores, am = self.search_full(log_probs, log_probs_length, n_best)
        if am is not None:
            scores = am
        tokens, n, scores = tokens.cpu().numpy(), n.cpu().numpy(), scores.cpu().numpy()
        return [[(float(scores[b, j]), self._text(tokens[b, j, :n[b, j]])) for j in range(n_best) if n[b, j] >= 0]
                for b in range(tokens.shape[0])]
