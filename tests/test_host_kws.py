"""CPU tier of CTC keyword search: the numpy oracle (tests/helpers/kws_oracle.py) against exhaustive enumeration, the picking
rules on hand-built traces, the C ABI's argument checks without a GPU, the ops layer's refusals and the pure record functions
of lightning_asr_amd/kws.py."""
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
import kws_oracle as K  # noqa: E402
from lightning_asr_amd import kws as kws_records  # noqa: E402  (the oracle is the definition of what this module reports)

assert K.MAX_LABELS == 64 and callable(kws_records.hit_records)


# ------------------------------------------------------------------------------------------------ oracle vs brute force
def test_oracle_matches_brute_force():
    """every T <= 6 and every phrase of L <= 3 labels over two labels plus blank: E_t and S_t of the oracle EQUAL the enumerated
    ones - the best score over every window and every frame labelling that starts in l_0, ends in l_{L-1} and collapses to the
    phrase, and the smallest start among the labellings that attain it.

    Exact equality, no tolerance: the emissions are log-softmaxed normals rounded to multiples of 2^-10, so every e_t and every
    partial sum (below 2^7 with 10 fractional bits) is exact in f32 and the f32 recursion IS the f64 sum of its path.  Every
    other row repeats the row before it, which makes exact ties between windows; the start rule runs through them."""
    C, blank = 3, 2
    rng = np.random.RandomState(0)
    n_cases = n_live = n_dead = n_tied = 0
    for T in range(1, 7):
        for L in range(1, 4):
            for phrase in itertools.product(range(2), repeat=L):
                lp = torch.log_softmax(torch.from_numpy(rng.randn(T, C).astype(np.float32) * 2.0), -1).numpy()
                lp = (np.round(lp * 1024.0) / 1024.0).astype(np.float32)
                for t in range(1, T, 2):
                    lp[t] = lp[t - 1]                                  # duplicated rows: forced ties
                E, S = K.search_one(lp, list(phrase), blank)
                Eb, Sb = K.brute_force(lp, list(phrase), blank)
                n_cases += 1
                assert E.dtype == np.float32 and np.array_equal(E.astype(np.float64), Eb), (T, phrase, E, Eb)
                assert np.array_equal(S.astype(np.int64), Sb), (T, phrase, S, Sb)
                n_live += int(np.isfinite(Eb).sum())
                n_dead += int((~np.isfinite(Eb)).sum())
                need = L + sum(1 for a, b in zip(phrase, phrase[1:]) if a == b)
                assert not np.isfinite(Eb[:need - 1]).any() and np.isfinite(Eb[need - 1:]).all()
                n_tied += int(len(set(Eb[np.isfinite(Eb)].tolist())) < int(np.isfinite(Eb).sum()))
    print("brute force: %d cases, %d live end frames, %d dead, %d cases with tied end scores" % (n_cases, n_live, n_dead, n_tied))
    # the inputs cover what they are meant to: of the 294 end frames both kinds occur often, and ties occur
    assert n_cases == 84 and n_live >= 100 and n_dead >= 100 and n_tied >= 5


def test_oracle_start_and_end_rules_on_a_run_of_zeros():
    """a run of frames whose greedy class is the phrase's one label: e = 0 on every frame, so every window ties at 0: the start
    is the EARLIEST frame of the run for every end, and the best frame is the LATEST end"""
    blank = 2
    lp = np.log(np.array([[0.1, 0.1, 0.8]] * 2 + [[0.8, 0.1, 0.1]] * 4 + [[0.1, 0.1, 0.8]] * 2, np.float32))
    E, S = K.search_one(lp, [0], blank)
    assert E[2:6].tolist() == [0.0] * 4 and S[2:6].tolist() == [2] * 4
    assert (E[:2] < 0).all() and (E[6:] < 0).all()
    assert K.best_of(E, S) == (0.0, (2, 6))
    n, spans, scores = K.pick(E, S, np.float32(-0.5), 4)
    assert n == 1 and spans[0].tolist() == [2, 6] and scores[0] == 0.0     # the later candidate wins the tie: the longest span
    # a phrase longer than the clip: dead everywhere
    E, S = K.search_one(lp[:2], [0, 0], blank)                             # "aa" needs 3 frames
    assert (E == -np.inf).all() and (S == -1).all() and K.best_of(E, S) == (-np.inf, (-1, -1))


# ------------------------------------------------------------------------------------------------ picking
def _trace(T, hits):
    E = np.full(T, -np.inf, np.float32)
    S = np.full(T, -1, np.int32)
    for t, (s, v) in hits.items():
        E[t], S[t] = v, s
    return E, S


def test_pick_rules():
    thr = np.float32(-2.0)
    # an overlapping candidate replaces the pending hit when it is better, and not when it is worse
    n, sp, sc = K.pick(*_trace(10, {3: (1, -1.5), 4: (1, -0.5), 5: (2, -1.0)}), thr, 4)
    assert n == 1 and sp[0].tolist() == [1, 5] and sc[0] == np.float32(-0.5)
    assert sp[1].tolist() == [-1, -1] and sc[1] == 0.0                     # unwritten slots
    # an equal score goes to the later candidate
    n, sp, sc = K.pick(*_trace(10, {3: (1, -1.0), 4: (1, -1.0)}), thr, 4)
    assert n == 1 and sp[0].tolist() == [1, 5]
    # candidates that do not overlap are both emitted (start == pending end is not an overlap)
    n, sp, sc = K.pick(*_trace(10, {3: (1, -1.0), 6: (4, -0.25)}), thr, 4)
    assert n == 2 and sp[:2].tolist() == [[1, 4], [4, 7]] and sc[:2].tolist() == [-1.0, -0.25]
    # more hits than slots: counted, the first max_hits stored
    n, sp, sc = K.pick(*_trace(12, {1: (0, -1.0), 4: (3, -0.5), 8: (6, -0.75)}), thr, 2)
    assert n == 3 and sp.tolist() == [[0, 2], [3, 5]] and sc.tolist() == [-1.0, -0.5]
    # E_t == thr exactly is a candidate; just below is not
    n, sp, sc = K.pick(*_trace(6, {2: (0, -2.0), 5: (4, np.nextafter(np.float32(-2.0), np.float32(-3.0)))}), thr, 4)
    assert n == 1 and sp[0].tolist() == [0, 3] and sc[0] == np.float32(-2.0)
    # nothing passes: no hit
    n, sp, sc = K.pick(*_trace(6, {2: (0, -2.5)}), thr, 4)
    assert n == 0 and (sp == -1).all() and (sc == 0).all()


def test_search_batch_clamps_and_threshold_per_label():
    """thr = threshold * L in f32; lengths, offsets and labels outside their ranges are clamped as the device clamps them"""
    rng = np.random.RandomState(1)
    lp = torch.log_softmax(torch.from_numpy(rng.randn(2, 12, 5).astype(np.float32)), -1).numpy()
    labels, offsets = [0, 1, 2, 3, 1], [0, 2, 5]
    out = K.search_batch(lp, [12, 5], 4, labels, offsets, 3, -1.0, 3)
    E, S = K.search_one(lp[1, :5], (2, 3, 1), 4)
    n, sp, sc = K.pick(E, S, np.float32(-1.0) * np.float32(3), 3)
    assert out[0][1, 1] == n and np.array_equal(out[1][1, 1], sp) and np.array_equal(out[2][1, 1], sc)
    assert out[3][1, 1] == K.best_of(E, S)[0]
    # L_max = 2 cuts the second phrase to its first two labels; a label of 9 is read as C - 1; in_lens -3 as 0, 99 as T
    cut = K.search_batch(lp, [99, -3], 4, [0, 1, 2, 9, 1], offsets, 2, -1.0, 3)
    E, S = K.search_one(lp[0], (2, 4), 4)
    assert cut[3][0, 1] == K.best_of(E, S)[0] and cut[3][1, 1] == -np.inf and cut[4][1, 1].tolist() == [-1, -1]
    assert (cut[0][1] == 0).all()


# ------------------------------------------------------------------------------------------------ C ABI without a GPU
def test_kws_abi_error_convention_without_gpu():
    from lightning_asr_amd import _lib
    lib = _lib.load()
    assert lib.lasr_version() >= 113
    E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
    rc = lib.lasr_ctc_kws(None, None, 1, 4, 3, 2, None, None, 1, 1, -2.0, 1, None, None, None, None, None, None, 0, None)
    assert rc == E_ARG and b"null pointer" in lib.lasr_last_error()
    # host buffers stand in for device pointers: every call below is refused before anything is launched
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(B=1, T=4, C=3, blank=2, K_=1, L_max=1, thr=-2.0, max_hits=1, ws_bytes=1 << 20, **null):
        ptr = {n: (None if n in null else p) for n in ("logp", "labels", "offsets", "n_hits", "span", "score", "best", "bspan", "ws")}
        return lib.lasr_ctc_kws(ptr["logp"], None, B, T, C, blank, ptr["labels"], ptr["offsets"], K_, L_max, thr, max_hits, ptr["n_hits"],
                                ptr["span"], ptr["score"], ptr["best"], ptr["bspan"], ptr["ws"], ws_bytes, None)

    for name in ("logp", "labels", "offsets", "n_hits", "span", "score", "best", "bspan", "ws"):
        assert call(**{name: None}) == E_ARG, name
    assert call(L_max=0) == E_SHAPE and b"64" in lib.lasr_last_error()
    assert call(L_max=65) == E_SHAPE and b"64" in lib.lasr_last_error()
    assert call(K_=0) == E_SHAPE
    assert call(max_hits=0) == E_SHAPE
    assert call(blank=3) == E_SHAPE and call(blank=-1) == E_SHAPE
    assert call(T=1 << 20, C=1 << 11) == E_SHAPE                       # T * C = 2^31
    for thr in (0.1, -1e6, float("nan"), -float("inf")):
        assert call(thr=thr) == E_ARG and b"threshold" in lib.lasr_last_error(), thr
    need = lib.lasr_ctc_kws_workspace_bytes(2, 501, 9)
    assert need >= 2 * 501 * 4 and lib.lasr_ctc_kws_workspace_bytes(0, 4, 1) == 0
    assert call(B=2, T=501, K_=9, ws_bytes=need - 1) == E_WORKSPACE and b"workspace" in lib.lasr_last_error()
    assert "lasr_ctc_kws" in _lib.SIGNATURES and "lasr_ctc_kws_workspace_bytes" in _lib.SIGNATURES


def test_ops_refusals():
    from lightning_asr_amd import _lib, ops
    assert ops.KWS_MAX_LABELS == 64
    kw = dict(n_classes=5, blank=4, device="cpu")
    for bad in ([], [[]], [[0], []], [[0] * 65], [[0, 4]], [[5]], [[-1]]):
        with pytest.raises(ValueError):
            ops.build_keywords(bad, **kw)
    with pytest.raises(ValueError, match="phrase 1"):
        ops.build_keywords([[0], [1, 4]], **kw)
    bank = ops.build_keywords([[0, 1], [2], [0, 1]], **kw)
    assert bank.n_phrases == 3 and bank.max_len == 2 and bank.lengths == [2, 1, 2]
    assert bank.labels.tolist() == [0, 1, 2, 0, 1] and bank.offsets.tolist() == [0, 2, 3, 5]
    assert bank.labels.dtype == torch.int32 and bank.offsets.dtype == torch.int32
    assert ops.build_keywords([[0] * 64], **kw).max_len == 64
    logp = torch.zeros(1, 4, 5).log_softmax(-1)
    with pytest.raises(_lib.LasrError):                                 # CPU tensors are refused, never emulated
        ops.ctc_keyword_search(logp, None, 4, bank)
    with pytest.raises(ValueError):
        ops.ctc_keyword_search(logp.double(), None, 4, bank)
    with pytest.raises(ValueError):
        ops.ctc_keyword_search(logp, None, 3, bank)                     # not the bank's blank
    with pytest.raises(ValueError):
        ops.ctc_keyword_search(torch.zeros(1, 4, 6), None, 4, bank)     # not the bank's classes
    with pytest.raises(ValueError):
        ops.ctc_keyword_search(logp, torch.tensor([4]), 4, bank)        # int64 lens
    with pytest.raises(ValueError):
        ops.ctc_keyword_search(logp, None, 4, bank, max_hits=0)
    with pytest.raises(TypeError):
        ops.ctc_keyword_search(logp, None, 4, [[0, 1]])


# ------------------------------------------------------------------------------------------------ spans -> records
def test_hit_records_on_fixed_numbers():
    from lightning_asr_amd import kws
    import lightning_asr_amd
    assert lightning_asr_amd.kws is kws
    keywords, lengths = ["hey", "ok", "hey"], [3, 2, 3]
    n_hits = [2, 3, 0]                                                  # "ok": three hits, two slots
    span = [[[10, 20], [40, 60]], [[10, 14], [2, 5]], [[-1, -1], [-1, -1]]]
    score = [[-1.5, 0.0], [-0.5, -1.0], [0.0, 0.0]]
    recs = kws.hit_records(keywords, lengths, n_hits, span, score, 0.02, duration=1.0)
    assert [(r["keyword"], r["start"], r["end"]) for r in recs] == [
        ("ok", pytest.approx(0.04), pytest.approx(0.10)), ("hey", pytest.approx(0.20), pytest.approx(0.40)),
        ("ok", pytest.approx(0.20), pytest.approx(0.28)), ("hey", pytest.approx(0.80), pytest.approx(1.0))]   # 60 * 0.02 = 1.2, clipped
    assert set(recs[0]) == {"keyword", "start", "end", "score", "score_per_label", "confidence"}
    assert recs[1]["score"] == -1.5 and recs[1]["score_per_label"] == pytest.approx(-0.5)
    assert recs[1]["confidence"] == pytest.approx(math.exp(-0.5))
    assert recs[3]["score"] == 0.0 and recs[3]["confidence"] == 1.0
    assert recs[0]["score_per_label"] == pytest.approx(-0.5) and recs[2]["score_per_label"] == pytest.approx(-0.25)
    # a hit in the clip's last frame: both times clipped to the duration
    last = kws.hit_records(["hey"], [3], [1], [[[50, 51]]], [[-0.3]], 0.02, duration=1.0)
    assert last[0]["start"] == 1.0 and last[0]["end"] == 1.0
    assert kws.hit_records(["a"], [1], [0], [[[-1, -1]]], [[0.0]], 0.02) == []
    with pytest.raises(ValueError):
        kws.hit_records(["a"], [1], [1], [[[-1, -1]]], [[0.0]], 0.02)   # a counted hit without a span
    with pytest.raises(ValueError):
        kws.hit_records(["a", "b"], [1], [0], [[[-1, -1]]], [[0.0]], 0.02)
    sc = kws.score_records(["hey", "ok"], [3, 2], [-1.5, -math.inf], [[10, 20], [-1, -1]], 0.02, duration=0.3)
    assert sc[0] == {"keyword": "hey", "score_per_label": pytest.approx(-0.5), "start": pytest.approx(0.2), "end": pytest.approx(0.3)}
    assert sc[1] == {"keyword": "ok", "score_per_label": -math.inf, "start": None, "end": None}
