"""CPU tier of CTC forced alignment: the numpy oracle (tests/helpers/ctc_align_oracle.py) against brute force, the C ABI's
argument checks without a GPU, and the pure span-to-record functions of lightning_asr_amd/align.py."""
import ctypes
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ctc_align_oracle as A  # noqa: E402


# ------------------------------------------------------------------------------------------------ oracle vs brute force
def test_oracle_matches_brute_force():
    """every T <= 6 and every target of S <= 3 labels over a 3-class alphabet (two labels + blank), repeats included: the
    oracle's path is a lattice path that collapses to the target, its score is the maximum over ALL alignments (enumerated,
    f64) to 1e-6, and it reports infeasible exactly where no alignment exists.

    The emissions are log-softmaxed normals rounded to multiples of 2^-10.  The oracle scores in f32 by definition, and six f32
    additions at |score| ~ 16 (ulp 1.9e-6) cannot be held to an absolute 1e-6 against f64; on the 2^-10 grid every partial sum
    (below 2^7, 10 fractional bits) is exact in f32, so the oracle's score IS the f64 sum of its path and any distance from the
    enumerated maximum is a mistake of the recursion, not rounding.  The grid also produces exact ties, which the path checks
    then run through."""
    C, blank = 3, 2
    rng = np.random.RandomState(0)
    n_feasible = n_infeasible = 0
    for T in range(0, 7):
        for S in range(0, 4):
            for target in itertools.product(range(2), repeat=S):
                lp = torch.log_softmax(torch.from_numpy(rng.randn(T, C).astype(np.float32) * 2.0), -1).numpy() if T else np.zeros((0, C), np.float32)
                lp = (np.round(lp * 1024.0) / 1024.0).astype(np.float32)
                best, n = A.brute_force(lp, list(target), blank)
                score, states = A.align_one(lp, list(target), blank)
                if n == 0:
                    n_infeasible += 1
                    assert states is None and score == -np.inf, (T, target)
                    repeats = sum(1 for a, b in zip(target, target[1:]) if a == b)
                    assert T < S + repeats
                    continue
                n_feasible += 1
                assert states is not None and len(states) == T, (T, target)
                if T:
                    assert A.valid_path(states, S), (T, target, states)
                assert A.collapse(states, list(target), blank) == list(target)
                assert abs(float(score) - best) <= 1e-6, (T, target, float(score), best)
                path_sum = sum(float(lp[t, target[s >> 1] if s & 1 else blank]) for t, s in enumerate(states))
                assert abs(path_sum - best) <= 1e-6
    assert n_feasible > 50 and n_infeasible > 20


def test_oracle_tie_rule_and_batch_outputs():
    """uniform emissions make every alignment tie: stay is preferred over step over skip walking backwards, and the end state
    is the blank 2S - so the labels sit as EARLY as the ties allow and trailing frames are blank"""
    T, C, blank = 6, 3, 2
    lp = np.full((1, T, C), math.log(1.0 / 3.0), np.float32)
    score, st, flp, ls, le = A.align_batch(lp, [[0, 1]], None, [2], blank)
    # backwards from state 4 (blank): stay while it ties, so the path is 1 3 4 4 4 4
    assert st[0].tolist() == [1, 3, 4, 4, 4, 4]
    assert ls[0].tolist() == [0, 1] and le[0].tolist() == [1, 2]
    assert abs(float(score[0]) - 6 * math.log(1 / 3)) < 1e-5 and abs(float(flp[0].sum()) - float(score[0])) < 1e-5
    # ragged fills: frames past in_lens are -1 / 0, labels past tgt_lens are -1, an infeasible row is -1 everywhere
    lp2 = np.repeat(lp, 3, axis=0)
    score, st, flp, ls, le = A.align_batch(lp2, [[0, 1, 1], [0, 0, 0], [1, 0, 0]], [4, 4, 0], [1, 3, 0], blank)
    assert st[0].tolist() == [1, 2, 2, 2, -1, -1] and flp[0, 4:].tolist() == [0.0, 0.0]
    assert ls[0].tolist() == [0, -1, -1] and le[0].tolist() == [1, -1, -1]
    assert score[1] == -np.inf and (st[1] == -1).all() and (ls[1] == -1).all() and (flp[1] == 0).all()    # 4 < 3 + 2 repeats
    assert score[2] == 0.0 and (st[2] == -1).all() and (ls[2] == -1).all()                                 # no frame, no label


# ------------------------------------------------------------------------------------------------ C ABI without a GPU
def test_align_abi_error_convention_without_gpu():
    from lightning_asr_amd import _lib, ops
    lib = _lib.load()
    assert lib.lasr_version() >= 105
    E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
    rc = lib.lasr_ctc_align(None, None, None, None, 1, 4, 3, 1, 2, None, None, None, None, None, None, 0, None)
    assert rc == E_ARG and b"null pointer" in lib.lasr_last_error()
    # host buffers stand in for device pointers: every call below is refused before anything is launched
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(B, T, C, S_max, blank, ws_bytes):
        return lib.lasr_ctc_align(p, p, None, p, B, T, C, S_max, blank, p, p, p, p, p, p, ws_bytes, None)

    assert lib.lasr_ctc_align_workspace_bytes(1, 4, 2048) == 0
    assert lib.lasr_ctc_align_workspace_bytes(1, 4, 2047) > 0
    assert lib.lasr_ctc_align_workspace_bytes(2, 501, 0) > 0
    assert call(1, 4, 3, 2048, 2, 1 << 30) == E_SHAPE and b"2048" in lib.lasr_last_error()
    need = lib.lasr_ctc_align_workspace_bytes(1, 4, 1)
    assert call(1, 4, 3, 1, 2, need - 1) == E_WORKSPACE and b"workspace" in lib.lasr_last_error()
    assert call(1, 4, 3, 1, 3, need) == E_SHAPE                       # blank >= C
    assert call(1, 4, 3, 1, -1, need) == E_SHAPE
    assert lib.lasr_ctc_align(p, None, None, p, 1, 4, 3, 1, 2, p, p, p, p, p, p, need, None) == E_ARG   # targets with S_max > 0
    # ops: CPU tensors are refused, never emulated; bad labels are a ValueError before any launch
    logp = torch.zeros(1, 4, 3).log_softmax(-1)
    tl = torch.tensor([2], dtype=torch.int32)
    with pytest.raises(_lib.LasrError):
        ops.ctc_align(logp, torch.tensor([[0, 1]]), None, tl, 2)
    with pytest.raises(ValueError):
        ops.ctc_align(logp, torch.tensor([[0, 2]]), None, tl, 2)      # the blank inside the targets
    with pytest.raises(ValueError):
        ops.ctc_align(logp, torch.tensor([[0, 3]]), None, tl, 2)      # outside [0, C)
    with pytest.raises(_lib.LasrError):
        ops.ctc_align(logp, torch.tensor([[0, 2]]), None, torch.tensor([1], dtype=torch.int32), 2)   # ... but only within tgt_lens
    with pytest.raises(ValueError):
        ops.ctc_align(logp, torch.zeros(1, ops.CTC_MAX_LABELS + 1, dtype=torch.int64), None, tl, 2)
    with pytest.raises(ValueError):
        ops.ctc_align(logp.double(), torch.tensor([[0, 1]]), None, tl, 2)
    with pytest.raises(ValueError):
        ops.ctc_align(logp, torch.tensor([[0, 1]], dtype=torch.int32), None, tl, 2)
    with pytest.raises(ValueError):
        ops.ctc_align(logp, torch.tensor([[0, 1]]), None, torch.tensor([2, 2], dtype=torch.int32), 2)


# ------------------------------------------------------------------------------------------------ spans -> records
EN = [" ", "'"] + [chr(ord("a") + i) for i in range(26)]


def _ids(text, labels):
    return [labels.index(c) for c in text]


def test_records_english_words_and_clipping():
    from lightning_asr_amd import align as AL
    import lightning_asr_amd
    assert lightning_asr_amd.unit_records is AL.unit_records and lightning_asr_amd.align is AL
    assert AL.frame_seconds(160, 16000, 2) == pytest.approx(0.02)
    assert AL.frame_seconds(160, 16000, 4) == pytest.approx(0.04)
    with pytest.raises(ValueError):
        AL.frame_seconds(0, 16000, 2)
    # "hi yo": frames  0 1 | h 2 3 | blank 4 | i 5 (one frame) | blank 6 | ' ' 7 | y 8 9 | o 10 11 12 | blank 13 14
    text = "hi yo"
    ids = _ids(text, EN)
    start = [2, 5, 7, 8, 10]
    end = [4, 6, 8, 10, 13]
    flp = [math.log(0.5)] * 15
    flp[2], flp[3] = math.log(0.9), math.log(0.4)
    flp[5] = math.log(0.25)
    labs = AL.label_records(ids, start, end, flp, EN, 0.02, duration=0.25)
    assert [r["label"] for r in labs] == list(text)
    assert labs[0]["start"] == pytest.approx(0.04) and labs[0]["end"] == pytest.approx(0.08)
    assert labs[0]["score"] == pytest.approx(math.sqrt(0.9 * 0.4))
    assert labs[1]["start"] == pytest.approx(0.10) and labs[1]["end"] == pytest.approx(0.12)       # a one-frame label
    assert labs[1]["score"] == pytest.approx(0.25)
    assert labs[4]["start"] == pytest.approx(0.20) and labs[4]["end"] == pytest.approx(0.25)       # 13 * 0.02 = 0.26, clipped
    words = AL.unit_records(ids, start, end, flp, EN, 0.02, duration=0.25)
    assert [w["word"] for w in words] == ["hi", "yo"]
    assert [[r["label"] for r in w["labels"]] for w in words] == [["h", "i"], ["y", "o"]]          # the space is in no word
    # leading blanks (frames 0-1) and trailing blanks (13-14) belong to no word; nor does the space's frame 7
    assert words[0]["start"] == pytest.approx(0.04) and words[0]["end"] == pytest.approx(0.12)
    assert words[1]["start"] == pytest.approx(0.16) and words[1]["end"] == pytest.approx(0.25)
    # a word's score runs over its whole span, the blank between h and i included: frames 2..5
    assert words[0]["score"] == pytest.approx(math.exp((math.log(0.9) + math.log(0.4) + math.log(0.5) + math.log(0.25)) / 4))
    assert words[1]["score"] == pytest.approx(0.5)
    for a, b in zip(words, words[1:]):
        assert a["end"] <= b["start"]
    # without a duration nothing is clipped
    assert AL.unit_records(ids, start, end, flp, EN, 0.02)[1]["end"] == pytest.approx(0.26)
    # leading / trailing / doubled spaces make no empty word
    ids2 = _ids(" a  b ", EN)
    w2 = AL.unit_records(ids2, [0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6], [0.0] * 6, EN, 0.02)
    assert [w["word"] for w in w2] == ["a", "b"] and w2[0]["score"] == pytest.approx(1.0)
    assert AL.unit_records([], [], [], flp, EN, 0.02) == []
    with pytest.raises(ValueError):
        AL.unit_records(ids, [-1] * 5, [-1] * 5, flp, EN, 0.02)                                     # an infeasible row's spans


def test_records_vocabulary_without_space():
    """no space label (AISHELL): every label is its own unit"""
    from lightning_asr_amd import align as AL
    labels = ["你", "好", "吗"]
    ids = [0, 1, 1, 2]
    start, end = [1, 3, 6, 7], [3, 5, 7, 9]
    flp = [math.log(0.5)] * 10
    units = AL.unit_records(ids, start, end, flp, labels, 0.04, duration=10.0)
    assert [u["word"] for u in units] == ["你", "好", "好", "吗"]
    assert all(len(u["labels"]) == 1 and u["labels"][0]["label"] == u["word"] for u in units)
    assert [u["start"] for u in units] == pytest.approx([0.04, 0.12, 0.24, 0.28])
    assert [u["end"] for u in units] == pytest.approx([0.12, 0.20, 0.28, 0.36])
    assert all(u["score"] == pytest.approx(0.5) for u in units)
    assert AL.word_records is AL.unit_records
