"""Host side of CTC forced alignment: what ``ops.ctc_align`` returns for one utterance (label spans in frames, per-frame
log-probs) -> per-label and per-word records in seconds.  Pure functions over plain sequences: no device, no torch.

Times are ``frame * frame_seconds`` clipped to the clip's duration; ``frame_seconds`` is the hop of the feature front-end
times the model's time stride over the sample rate (``frame_seconds`` below), 0.02 s for the shipped variants (160 samples at
16 kHz, stride 2).  A score is exp(mean frame log-prob) over the frames of the span: for a label its own frames, for a word
the frames from its first label's first frame to its last label's last, the blanks inside it included.  The blank frames
between two labels belong to neither label.

For long recordings (``AsrTranslator.align_long`` / ``cut_corpus``): ``sentence_records`` turns one alignment of many sentences
into word and sentence records, ``group_sentences`` / ``cut_samples`` cut the recording into training utterances, and
``window_batches`` / ``window_frame_offsets`` arrange the overlapping windows of ``encode_long``."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

__all__ = ["frame_seconds", "label_records", "unit_records", "word_records", "sentence_records", "group_sentences", "cut_samples",
           "window_batches", "window_frame_offsets"]


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


# ---------------------------------------------------------------------------------------------- long recordings
def sentence_records(sentence_ids: Sequence[Sequence[int]], label_start: Sequence[int], label_end: Sequence[int],
                     frame_logp: Sequence[float], labels: Sequence[str], frame_secs: float, duration: Optional[float] = None,
                     sep: int = 0):
    """One alignment of several sentences -> (words, sentences).  The alignment's targets are the sentences' label ids one after
    the other with ``sep`` labels between two of them (the space that joins them; it belongs to no word and no sentence).
    words: the ``unit_records`` of every sentence, in order.  sentences: one {"text", "start", "end", "score", "min_word_score",
    "first_word", "n_words"} each - start / end: its first label's first frame and its last label's last, in seconds;
    score = exp(mean frame log-prob) over those frames, blanks included; min_word_score: the lowest score of its words
    (its own score when it has no word); first_word / n_words: its slice of ``words``."""
    words: List[dict] = []
    sents: List[dict] = []
    pos = 0
    for k, ids in enumerate(sentence_ids):
        if len(ids) == 0:
            raise ValueError("sentence %d has no labels" % k)
        a, b = pos, pos + len(ids)
        pos = b + int(sep)
        w = unit_records(ids, label_start[a:b], label_end[a:b], frame_logp, labels, frame_secs, duration)
        s, e = int(label_start[a]), int(label_end[b - 1])
        score = _span_score(frame_logp, s, e)
        sents.append({"text": "".join(labels[int(c)] for c in ids), "start": _time(s, frame_secs, duration),
                      "end": _time(e, frame_secs, duration), "score": score,
                      "min_word_score": min([r["score"] for r in w]) if w else score, "first_word": len(words), "n_words": len(w)})
        words.extend(w)
    return words, sents


def group_sentences(sentences: Sequence[dict], max_duration: float, duration: float, joiner: str = " ", pad: float = 0.5):
    """Consecutive sentence records (``sentence_records``) -> (groups, dropped): utterances of at most ``max_duration`` seconds.
    The recording is cut in the middle of the gap between two neighbouring sentences; before the first sentence and after the last
    it is cut ``pad`` seconds away from them (inside [0, duration]).  Grouping is greedy: a group takes the next sentence while
    the span between its outer cuts stays within max_duration.  A sentence that is longer on its own is dropped.
    groups: [{"first", "last" (sentence indices, inclusive), "start", "end" (the cuts, seconds), "text" (the texts joined by
    ``joiner``), "min_word_score" (the lowest of its sentences')}]; dropped: the indices of the sentences no group holds."""
    n = len(sentences)
    if n == 0:
        return [], []
    if max_duration <= 0:
        raise ValueError("group_sentences: max_duration must be positive")
    cuts = [max(0.0, float(sentences[0]["start"]) - pad)]
    for i in range(1, n):
        cuts.append(0.5 * (float(sentences[i - 1]["end"]) + float(sentences[i]["start"])))
    cuts.append(min(float(duration), float(sentences[-1]["end"]) + pad))
    groups, dropped = [], []
    i = 0
    while i < n:
        if cuts[i + 1] - cuts[i] > max_duration:
            dropped.append(i)
            i += 1
            continue
        j = i
        while j + 1 < n and cuts[j + 2] - cuts[i] <= max_duration:
            j += 1
        groups.append({"first": i, "last": j, "start": cuts[i], "end": cuts[j + 1],
                       "text": joiner.join(sentences[k]["text"] for k in range(i, j + 1)),
                       "min_word_score": min(float(sentences[k]["min_word_score"]) for k in range(i, j + 1))})
        i = j + 1
    return groups, dropped


def cut_samples(groups: Sequence[dict], sample_rate: int, total_samples: int, max_duration: float) -> List[tuple]:
    """the sample spans [(start, end), ...] of ``group_sentences`` groups: the cuts rounded to samples inside [0, total_samples]
    (two groups that share a cut share the sample), an end pulled in where rounding would pass max_duration"""
    out = []
    most = int(math.floor(float(max_duration) * sample_rate))
    for g in groups:
        s = min(max(int(round(float(g["start"]) * sample_rate)), 0), int(total_samples))
        e = min(max(int(round(float(g["end"]) * sample_rate)), s), int(total_samples))
        out.append((s, min(e, s + most)))
    return out


def window_batches(windows: Sequence[tuple], batch_size: int) -> List[List[int]]:
    """``streaming.plan_windows`` windows -> batches of window indices for one forward each: windows of equal sample length
    together, at most ``batch_size`` of them, in time order inside a batch; lengths in the order they first occur (a length that
    occurs once - the first and the last window - is a batch of its own)"""
    if int(batch_size) < 1:
        raise ValueError("window_batches: batch_size must be at least 1")
    by_len: dict = {}
    for i, w in enumerate(windows):
        by_len.setdefault(int(w[1]) - int(w[0]), []).append(i)
    out = []
    for idx in by_len.values():
        for k in range(0, len(idx), int(batch_size)):
            out.append(idx[k:k + int(batch_size)])
    return out


def window_frame_offsets(windows: Sequence[tuple], total_frames: int, frame_samples: int) -> List[int]:
    """the recording's frame at which each window's emitted rows start; ValueError unless the windows tile [0, total_frames)
    exactly once, in order"""
    offs, pos = [], 0
    for s0, _, first, n in windows:
        off = int(s0) // int(frame_samples) + int(first)
        if off != pos or int(n) <= 0:
            raise ValueError("windows do not tile the recording: a window emits frames %d.. where %d is next" % (off, pos))
        offs.append(off)
        pos += int(n)
    if pos != int(total_frames):
        raise ValueError("windows emit %d frames of %d" % (pos, int(total_frames)))
    return offs
