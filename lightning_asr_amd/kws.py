"""Host side of CTC keyword search: what ``ops.ctc_keyword_search`` returns for one utterance (hit spans in frames, scores)
-> records in seconds.  Pure functions over plain sequences: no device, no torch.

A hit's ``score`` is the log-likelihood ratio of the phrase's best path over the span against the greedy path over the same
frames (<= 0, 0 when the phrase IS the greedy path there); ``score_per_label`` divides it by the phrase's labels - the unit the
threshold is given in - and ``confidence`` is its exp, in (0, 1].  Times are ``frame * frame_seconds`` clipped to the clip's
duration, as align.py's records."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

from .align import _time

__all__ = ["hit_records", "sort_records", "score_records"]


def sort_records(records: List[dict], keywords: Sequence[str]) -> List[dict]:
    """by start, then by the keyword's place in `keywords` (a keyword listed twice: its first place)"""
    order = {}
    for i, k in enumerate(keywords):
        order.setdefault(k, i)
    return sorted(records, key=lambda r: (r["start"], order[r["keyword"]]))


def hit_records(keywords: Sequence[str], lengths: Sequence[int], n_hits: Sequence[int], hit_span, hit_score, frame_secs: float,
                duration: Optional[float] = None) -> List[dict]:
    """one {"keyword", "start", "end", "score", "score_per_label", "confidence"} per hit of ONE utterance: keywords (K) the
    phrases' names, lengths (K) their label counts, n_hits (K), hit_span (K, max_hits, 2), hit_score (K, max_hits) that
    utterance's rows of KeywordHits as lists.  Of a pair with n_hits above max_hits the stored max_hits are returned.  Times are
    clipped to `duration` (a hit in the clip's last frame can start where it ends).  Sorted by start, then keyword order."""
    if not (len(keywords) == len(lengths) == len(n_hits) == len(hit_span) == len(hit_score)):
        raise ValueError("hit_records: %d keywords, %d lengths, %d / %d / %d result rows"
                         % (len(keywords), len(lengths), len(n_hits), len(hit_span), len(hit_score)))
    out = []
    for k, name in enumerate(keywords):
        L = int(lengths[k])
        if L < 1:
            raise ValueError("hit_records: keyword %d has %d labels" % (k, L))
        for i in range(min(int(n_hits[k]), len(hit_score[k]))):
            s, e = int(hit_span[k][i][0]), int(hit_span[k][i][1])
            if s < 0 or e <= s:
                raise ValueError("hit_records: hit %d of keyword %d has no span (start %d, end %d)" % (i, k, s, e))
            score = float(hit_score[k][i])
            out.append({"keyword": name, "start": _time(s, frame_secs, duration), "end": _time(e, frame_secs, duration),
                        "score": score, "score_per_label": score / L, "confidence": math.exp(score / L)})
    return sort_records(out, keywords)


def score_records(keywords: Sequence[str], lengths: Sequence[int], best_score: Sequence[float], best_span, frame_secs: float,
                  duration: Optional[float] = None) -> List[dict]:
    """one {"keyword", "score_per_label", "start", "end"} per keyword, in keyword order: the best score of the phrase anywhere in
    the utterance over its labels, and where; -inf with start = end = None for a phrase that does not fit the clip"""
    out = []
    for k, name in enumerate(keywords):
        v = float(best_score[k])
        if math.isfinite(v):
            s, e = int(best_span[k][0]), int(best_span[k][1])
            out.append({"keyword": name, "score_per_label": v / int(lengths[k]), "start": _time(s, frame_secs, duration),
                        "end": _time(e, frame_secs, duration)})
        else:
            out.append({"keyword": name, "score_per_label": -math.inf, "start": None, "end": None})
    return out
