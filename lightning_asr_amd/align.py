"""Host side of CTC forced alignment: what ``ops.ctc_align`` returns for one utterance (label spans in frames, per-frame
log-probs) -> per-label and per-word records in seconds.  Pure functions over plain sequences: no device, no torch.

Times are ``frame * frame_seconds`` clipped to the clip's duration; ``frame_seconds`` is the hop of the feature front-end
times the model's time stride over the sample rate (``frame_seconds`` below), 0.02 s for the shipped variants (160 samples at
16 kHz, stride 2).  A score is exp(mean frame log-prob) over the frames of the span: for a label its own frames, for a word
the frames from its first label's first frame to its last label's last, the blanks inside it included.  The blank frames
between two labels belong to neither label."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

__all__ = ["frame_seconds", "label_records", "unit_records", "word_records"]


def frame_seconds(hop_length: int, sample_rate: int, time_stride: int) -> float:
    """seconds of audio one output frame of the model advances by"""
    if hop_length <= 0 or sample_rate <= 0 or time_stride <= 0:
        raise ValueError("frame_seconds: hop_length, sample_rate and time_stride must be positive")
    return float(hop_length) * float(time_stride) / float(sample_rate)


def _time(frame: int, frame_secs: float, duration: Optional[float]) -> float:
    t = frame * frame_secs
    if duration is not None:
        t = min(t, float(duration))
    return max(t, 0.0)


def _span_score(frame_logp: Sequence[float], start: int, end: int) -> float:
    n = end - start
    if n <= 0:
        return 0.0
    return math.exp(sum(float(frame_logp[t]) for t in range(start, end)) / n)


def label_records(targets: Sequence[int], label_start: Sequence[int], label_end: Sequence[int], frame_logp: Sequence[float],
                  labels: Sequence[str], frame_secs: float, duration: Optional[float] = None) -> List[dict]:
    """one {"label", "start", "end", "score"} per target label, in order"""
    out = []
    for i, c in enumerate(targets):
        s, e = int(label_start[i]), int(label_end[i])
        if s < 0 or e <= s:
            raise ValueError("label %d has no span (start %d, end %d): not a feasible alignment" % (i, s, e))
        out.append({"label": labels[int(c)], "start": _time(s, frame_secs, duration), "end": _time(e, frame_secs, duration),
                    "score": _span_score(frame_logp, s, e)})
    return out


def unit_records(targets: Sequence[int], label_start: Sequence[int], label_end: Sequence[int], frame_logp: Sequence[float],
                 labels: Sequence[str], frame_secs: float, duration: Optional[float] = None) -> List[dict]:
    """one {"word", "start", "end", "score", "labels": [label records]} per unit, by WER's rule: a vocabulary with a space label
    splits words at it (the space labels belong to no word, empty words are dropped); one without makes every label a unit."""
    recs = label_records(targets, label_start, label_end, frame_logp, labels, frame_secs, duration)
    has_space = " " in labels
    groups: List[List[int]] = []
    cur: List[int] = []
    for i, r in enumerate(recs):
        if has_space and r["label"] == " ":
            if cur:
                groups.append(cur)
            cur = []
        elif has_space:
            cur.append(i)
        else:
            groups.append([i])
    if cur:
        groups.append(cur)
    out = []
    for g in groups:
        s, e = int(label_start[g[0]]), int(label_end[g[-1]])
        out.append({"word": "".join(recs[i]["label"] for i in g), "start": _time(s, frame_secs, duration),
                    "end": _time(e, frame_secs, duration), "score": _span_score(frame_logp, s, e), "labels": [recs[i] for i in g]})
    return out


word_records = unit_records
