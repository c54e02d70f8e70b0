"""Host tier of the hotword biasing (no GPU): the f64 oracle (tests/helpers/ctc_beam_bias_oracle.py) against a brute-force reading
of the definition, the builder behind lasr_hotword_build (lightning_asr_amd/csrc/hotword_io.h) - error codes, node counts - and
lasr_hotword_score, the host walk over the image with the walker the kernels call, against the oracle, exactly.  Weights are
multiples of 0.25, so every credit and bonus is exact in f32 and the comparisons are ``==``."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ctc_beam_bias_oracle as BO  # noqa: E402
import ctc_beam_oracle as O  # noqa: E402

E_ARG, E_WORKSPACE, E_FORMAT = -1, -3, -4


def random_bank(rng, C, blank, n, max_len, alphabet=None):
    """n phrases over `alphabet` (default: every label but the blank); about a third are cut from or grown out of earlier
    ones, so that prefixes, extensions and shared suffixes occur"""
    labels = [c for c in (range(C) if alphabet is None else alphabet) if c != blank]
    phrases = []
    for _ in range(n):
        kind = rng.integers(0, 6)
        if phrases and kind == 0:
            p = list(phrases[rng.integers(len(phrases))])
            p = p[:max(1, rng.integers(1, len(p) + 1))]
        elif phrases and kind == 1:
            p = list(phrases[rng.integers(len(phrases))])[-2:] + [labels[rng.integers(len(labels))] for _ in range(rng.integers(0, 3))]
        else:
            p = [labels[rng.integers(len(labels))] for _ in range(rng.integers(1, max_len + 1))]
        phrases.append(p[:max_len])
    weights = [0.25 * int(rng.integers(1, 33)) for _ in range(n)]
    return phrases, weights


def random_sequence(rng, phrases, labels, n_parts):
    seq = []
    for _ in range(n_parts):
        kind = rng.integers(0, 3)
        if phrases and kind == 0:
            seq += phrases[rng.integers(len(phrases))]
        elif phrases and kind == 1:
            p = phrases[rng.integers(len(phrases))]
            seq += p[:rng.integers(1, len(p) + 1)]
        else:
            seq.append(labels[rng.integers(len(labels))])
    return [int(c) for c in seq]


def build(lib, phrases, weights, C, blank):
    labels = np.asarray([c for p in phrases for c in p], dtype=np.int32)
    off = np.zeros(len(phrases) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in phrases], out=off[1:])
    w = np.asarray(weights, dtype=np.float32)
    h = ctypes.c_void_p()
    rc = lib.lasr_hotword_build(labels.ctypes.data, off.ctypes.data, w.ctypes.data, len(phrases), C, blank, ctypes.byref(h))
    return rc, h


def info(lib, h):
    n, nodes, mc, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_float(), ctypes.c_size_t()
    assert lib.lasr_hotword_info(h, ctypes.byref(n), ctypes.byref(nodes), ctypes.byref(mc), ctypes.byref(nb)) == 0
    return n.value, nodes.value, mc.value, nb.value


def score(lib, h, seq):
    a = np.asarray(seq, dtype=np.int32)
    b, f, st = ctypes.c_float(), ctypes.c_float(), ctypes.c_int32()
    rc = lib.lasr_hotword_score(h, a.ctypes.data if a.size else None, a.size, ctypes.byref(b), ctypes.byref(f), ctypes.byref(st))
    assert rc == 0, lib.lasr_last_error()
    return b.value, f.value, st.value


@pytest.fixture(scope="module")
def lib():
    from lightning_asr_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_oracle_matches_brute_force_definition():
    rng = np.random.default_rng(0)
    seen = {k: 0 for k in BO.KINDS}
    for _ in range(300):
        phrases, weights = random_bank(rng, 5, 4, int(rng.integers(1, 6)), 4)
        bank = BO.Bank(phrases, weights)
        for _ in range(4):
            seq = random_sequence(rng, phrases, [0, 1, 2, 3], int(rng.integers(0, 6)))
            for n in range(len(seq) + 1):
                want = BO.brute_bonus(phrases, weights, tuple(seq[:n]))
                assert (bank.bonus(seq[:n]), bank.final(seq[:n])) == want, (phrases, weights, seq[:n])
        for k in BO.KINDS:
            seen[k] += bank.count[k]
    assert all(v > 0 for v in seen.values()), seen


def test_oracle_hand_worked_bank():
    # "ab" (w 2) inside "abc" (w 1), "bcd" (w 1.5), "e" (w 4); labels a..e = 1..5
    bank = BO.Bank([[1, 2, 3], [1, 2], [2, 3, 4], [5]], [1.0, 2.0, 1.5, 4.0])
    assert bank.n_nodes == 8 and bank.max_credit == 4.5
    assert [bank.bonus([1, 2, 3, 4, 5, 1, 2, 9, 1][:n]) for n in range(10)] == [0, 2, 4, 3, 3, 7, 9, 11, 11, 13]
    assert [bank.final([1, 2, 3, 4, 5, 1, 2, 9, 1][:n]) for n in range(10)] == [0, 0, 4, 3, 3, 7, 7, 11, 11, 11]
    # a b b c: the match of "ab" is banked when "b" fails, the suffix "b" of "bcd" is credited
    assert bank.bonus([1, 2, 2]) == 4 + 1.5 and bank.final([1, 2, 2]) == 4 and bank.final([1, 2, 2, 3, 4]) == 4 + 4.5


def test_search_with_everything_kept_is_likelihood_plus_final():
    """T = 5, C = 3, a beam that holds every labelling: each hypothesis scores its exact CTC log-likelihood + final(p)"""
    g = torch.Generator().manual_seed(3)
    lp = torch.log_softmax(torch.randn(5, 3, generator=g), -1).numpy().astype(np.float64)
    exact = O.brute_force(lp, 2)
    bank = BO.Bank([[0, 1], [1], [1, 1, 0]], [0.75, 0.5, 1.25])
    hyps, _, _ = BO.beam_search(lp, 5, 2, bank, 128, 3, 1.0, 128)
    assert len(hyps) == len(exact)
    for p, sc, am, fb in hyps:
        assert am == pytest.approx(exact[p], abs=1e-12) and fb == bank.final(p, count=False) and sc == pytest.approx(am + fb, abs=1e-12)
    best = max(exact, key=lambda p: exact[p] + bank.final(p, count=False))
    assert hyps[0][0] == best
    assert best != max(exact, key=lambda p: exact[p])             # the bias changes the winner on this input


def test_empty_bank_is_the_unbiased_oracle():
    g = torch.Generator().manual_seed(1)
    lp = torch.log_softmax(torch.randn(2, 30, 28, generator=g) * 3, -1).numpy()
    for W, k, cp in [(1, 40, 1.0), (16, 40, 1.0), (32, 8, 0.95)]:
        a, ma = O.beam_search_batch(lp, [30, 17], 27, W, k, cp, min(W, 4))
        b, mb, _ = BO.beam_search_batch(lp, [30, 17], 27, BO.Bank([], []), W, k, cp, min(W, 4))
        assert [[(p, s) for p, s in u] for u in a] == [[(p, s) for p, s, _, _ in u] for u in b]
        assert all(fb == 0.0 and am == s for u in b for _, s, am, fb in u)
        assert mb <= ma


# ------------------------------------------------------------------------------------------------ the C ABI
def test_build_error_codes_and_messages(lib):
    def err(phrases, weights, C=28, blank=27):
        rc, h = build(lib, phrases, weights, C, blank)
        assert not h.value
        return rc, lib.lasr_last_error().decode()
    rc, msg = err([[1, 2], [3, 28]], [1.0, 1.0])
    assert rc == E_ARG and "phrase 1" in msg and "28" in msg
    rc, msg = err([[1, 2], [3, -1]], [1.0, 1.0])
    assert rc == E_ARG and "phrase 1" in msg
    rc, msg = err([[27]], [1.0])
    assert rc == E_ARG and "phrase 0" in msg and "blank" in msg
    rc, msg = err([[1], [], [2]], [1.0, 1.0, 1.0])
    assert rc == E_ARG and "phrase 1" in msg and "empty" in msg
    rc, msg = err([[1], [2], list(range(1, 27)) + [1, 2, 3, 4, 5, 6, 7]], [1.0, 1.0, 1.0])
    assert rc == E_ARG and "phrase 2" in msg and "33" in msg
    for bad in (0.0, -1.0, math.inf, math.nan):
        rc, msg = err([[1], [2]], [1.0, bad])
        assert rc == E_ARG and "phrase 1" in msg and "weight" in msg
    rc, msg = err([[1]], [1.0], C=28, blank=28)
    assert rc == E_ARG and "blank" in msg
    # null pointers
    h = ctypes.c_void_p()
    assert lib.lasr_hotword_build(None, None, None, 1, 28, 27, ctypes.byref(h)) == E_ARG
    assert lib.lasr_hotword_build(None, None, None, 0, 28, 27, None) == E_ARG
    assert lib.lasr_hotword_info(None, None, None, None, None) == E_ARG
    assert lib.lasr_hotword_score(None, None, 0, None, None, None) == E_ARG
    # too many phrases, too many nodes: LASR_E_FORMAT
    rc, msg = err([[1]] * 65537, [1.0] * 65537)
    assert rc == E_FORMAT and "65536" in msg
    rng = np.random.default_rng(0)
    many = [[int(c) for c in rng.integers(0, 4000, 32)] for _ in range(40000)]        # ~ 1.28 M distinct nodes
    rc, msg = err(many, [1.0] * len(many), C=4334, blank=4333)
    assert rc == E_FORMAT and "trie nodes" in msg and "phrase" in msg


def test_build_node_counts_and_image(lib):
    cases = [
        ([], [], 1, 0.0),                                                       # the empty bank: the root alone
        ([[1, 2, 3], [1, 2], [1]], [1.0, 1.0, 1.0], 4, 3.0),                    # nested: one chain
        ([[1, 2], [1, 2], [1, 2]], [1.0, 3.0, 2.0], 3, 6.0),                    # duplicates: the largest weight counts
        ([[1, 2, 3], [4, 2, 3], [2, 3]], [1.0, 1.0, 0.5], 9, 3.0),              # shared suffixes share no node
        ([[1, 2, 3], [1, 2, 4], [1, 5]], [2.0, 1.0, 0.25], 6, 6.0),            # shared prefixes do
    ]
    for phrases, weights, nodes, mc in cases:
        if phrases:
            rc, h = build(lib, phrases, weights, 28, 27)
        else:                                                   # no phrases: the three arrays may be NULL
            h = ctypes.c_void_p()
            rc = lib.lasr_hotword_build(None, None, None, 0, 28, 27, ctypes.byref(h))
        assert rc == 0
        n, got_nodes, got_mc, nb = info(lib, h)
        assert (n, got_nodes, got_mc) == (len(phrases), nodes, mc), (phrases, n, got_nodes, got_mc)
        assert got_nodes == BO.Bank(phrases, weights).n_nodes
        # header + 16 bytes per node + a power-of-two table of 16-byte slots at load <= 1/2 (at least 16 slots)
        slots = (nb - 64 - 16 * nodes) // 16
        assert nb == 64 + 16 * nodes + 16 * slots and slots >= 16 and slots & (slots - 1) == 0 and slots >= 2 * (nodes - 1)
        buf = np.zeros(nb, dtype=np.uint8)
        assert lib.lasr_hotword_write_image(h, buf.ctypes.data, nb - 1) == E_WORKSPACE
        assert lib.lasr_hotword_write_image(h, buf.ctypes.data, nb) == 0
        assert buf[:4].tobytes() == b"ASHW"
        assert score(lib, h, []) == (0.0, 0.0, 0)
        lib.lasr_hotword_free(h)
    # the duplicate with the largest weight decides the credit
    rc, h = build(lib, [[1, 2], [1, 2]], [1.0, 3.0], 28, 27)
    assert score(lib, h, [1, 2]) == (6.0, 6.0, 0)
    # a label the bank cannot hold
    a = np.asarray([27], dtype=np.int32)
    assert lib.lasr_hotword_score(h, a.ctypes.data, 1, None, None, None) == E_ARG
    lib.lasr_hotword_free(h)


@pytest.mark.parametrize("C,alphabet", [(28, None), (4334, None), (4334, range(100, 112))])
def test_score_equals_oracle_exactly(lib, C, alphabet):
    """150 random banks x 4 random label sequences per class count: bonus, final and state after every label.  The third case
    draws a large-vocabulary bank from 12 labels, so that phrases overlap as they never would over 4333."""
    rng = np.random.default_rng(C + (0 if alphabet is None else 1))
    blank = C - 1
    labels = [c for c in (range(C) if alphabet is None else alphabet) if c != blank]
    seen = {k: 0 for k in BO.KINDS}
    for i in range(150):
        n = int(rng.integers(1, 40)) if i % 10 else 400
        phrases, weights = random_bank(rng, C, blank, n, 32 if i % 7 == 0 else 6, alphabet if alphabet is not None else
                                       (range(0, 6) if i % 3 == 0 else None))
        rc, h = build(lib, phrases, weights, C, blank)
        assert rc == 0, lib.lasr_last_error()
        bank = BO.Bank(phrases, weights)
        assert info(lib, h)[1:3] == (bank.n_nodes, bank.max_credit)
        for _ in range(4):
            seq = random_sequence(rng, phrases, labels if i % 3 else list(range(0, 6)), int(rng.integers(1, 12)))
            for m in range(len(seq) + 1):
                want = (bank.bonus(seq[:m]), bank.final(seq[:m]), bank.state(seq[:m]))
                assert score(lib, h, seq[:m]) == want, (phrases, weights, seq[:m])
        lib.lasr_hotword_free(h)
        for k in BO.KINDS:
            seen[k] += bank.count[k]
    assert all(v > 0 for v in seen.values()), seen


def test_ops_surface_without_gpu():
    from lightning_asr_amd import ops
    bank = ops.build_hotwords([[1, 2, 3], [1, 2], [2, 3, 4], [5]], [1.0, 2.0, 1.5, 4.0], n_classes=28, blank=27, device="cpu")
    assert (bank.n_phrases, bank.n_nodes, bank.max_credit) == (4, 8, 4.5) and bank.image.dtype == torch.uint8
    assert ops.hotword_bonus(bank, [1, 2, 3, 4, 5, 1, 2, 9, 1]) == (13.0, 11.0, 1)
    one = ops.build_hotwords([[1, 2]], n_classes=28, blank=27, device="cpu")           # the default weight
    assert ops.hotword_bonus(one, [1, 2]) == (4.0, 4.0, 0)
    assert "starting value" in ops.build_hotwords.__doc__
    empty = ops.build_hotwords([], n_classes=28, blank=27, device="cpu")
    assert (empty.n_phrases, empty.n_nodes, empty.max_credit) == (0, 1, 0.0)
    with pytest.raises(ValueError, match="phrase 1"):
        ops.build_hotwords([[1], [27]], n_classes=28, blank=27, device="cpu")
    with pytest.raises(ValueError, match="weights"):
        ops.build_hotwords([[1], [2]], [1.0], n_classes=28, blank=27, device="cpu")
    with pytest.raises(ValueError):
        ops.hotword_bonus(bank, [28])
    x = torch.zeros(1, 4, 28)
    with pytest.raises(TypeError):
        ops.ctc_beam_decode_biased(x, None, 27, None)
    with pytest.raises(ValueError, match="beam_width"):
        ops.ctc_beam_decode_biased(x, None, 27, bank, beam_width=129)
    with pytest.raises(ValueError, match="n_best"):
        ops.ctc_beam_decode_biased(x, None, 27, bank, beam_width=4, n_best=5)
    with pytest.raises(ValueError, match="built for 28 classes"):
        ops.ctc_beam_decode_biased(torch.zeros(1, 4, 29), None, 28, bank)


# ------------------------------------------------------------------------------------------------ the phrase parser
def test_parse_hotwords():
    from lightning_asr_amd.beam_search import parse_hotwords
    vocab = [" ", "'"] + [chr(ord("a") + i) for i in range(26)]
    assert parse_hotwords(vocab, ["ab", ("new york", 3.5), "it's"]) == ([[2, 3], [15, 6, 24, 0, 26, 16, 19, 12], [10, 21, 1, 20]],
                                                                       [2.0, 3.5, 2.0])
    assert parse_hotwords(vocab, ["ab"], 0.75)[1] == [0.75]
    assert parse_hotwords(["中", "文"], ["文中"]) == ([[1, 0]], [2.0])
    with pytest.raises(ValueError, match=r"hotword 1 \('café'\): character 'é'"):
        parse_hotwords(vocab, ["ok", "café"])
    with pytest.raises(ValueError, match="'new york'.*' '"):
        parse_hotwords(vocab[1:], ["new york"])              # a vocabulary without the " " label
    with pytest.raises(ValueError, match="hotword 0 is empty"):
        parse_hotwords(vocab, [""])
    with pytest.raises(TypeError):
        parse_hotwords(vocab, [3])
