"""CPU tier of the CTC beam search fused with a word-level LM: the word image behind lasr_arpa_load_words (n-gram sections and
the lexicon trie) read back byte by byte against a Python trie and ArpaOracle; the Python surface (ops.load_arpa picks the mode
by itself); the C ABI's argument errors; and the f64 oracle (tests/helpers/ctc_beam_wlm_oracle.py) against brute-force path
enumeration.  No GPU."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import arpa_synth as S  # noqa: E402
import ctc_beam_lm_oracle as LO  # noqa: E402
import ctc_beam_oracle as O  # noqa: E402
import ctc_beam_wlm_oracle as WO  # noqa: E402
import wlm_synth as WS  # noqa: E402

VOCAB = [" ", "a", "b", "c", "d"]
# words that are prefixes of others, doubled letters, and one the labels cannot spell
WORDS = ["a", "ab", "abc", "aa", "abba", "b", "bad", "cab", "dad", "add", "cad", "dab", "ax"]
WORD_MAGIC, CHAR_MAGIC = 0x574c5341, 0x4d4c5341
EMPTY = (1 << 64) - 1


def _lib():
    from lightning_asr_amd import _lib
    return _lib.load()


def _load_words(path, vocab, space_id):
    lib = _lib()
    words = [w.encode() for w in vocab]
    arr = (ctypes.c_char_p * max(len(words), 1))(*words)
    h = ctypes.c_void_p()
    rc = lib.lasr_arpa_load_words(str(path).encode(), ctypes.cast(arr, ctypes.c_void_p), len(words), space_id, ctypes.byref(h))
    return rc, h, lib.lasr_last_error().decode()


def _image(h):
    """(order, char_based, n_ngrams, (n_lexicon_words, n_nodes, n_dropped_words), image bytes); frees the handle"""
    lib = _lib()
    order, cb, n, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_size_t()
    assert lib.lasr_arpa_info(h, ctypes.byref(order), ctypes.byref(cb), ctypes.byref(n), ctypes.byref(nb)) == 0
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.lasr_arpa_lexicon_info(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    buf = np.zeros(nb.value, dtype=np.uint8)
    assert lib.lasr_arpa_write_image(h, buf.ctypes.data, nb.value) == 0
    lib.lasr_arpa_free(h)
    return order.value, cb.value, n.value, (a.value, b.value, c.value), buf.tobytes()


def _mix(k):
    M = (1 << 64) - 1
    k = ((k ^ (k >> 30)) * 0xbf58476d1ce4e5b9) & M
    k = ((k ^ (k >> 27)) * 0x94d049bb133111eb) & M
    return k ^ (k >> 31)


class Image:
    """a word image, read the way the kernel reads it"""

    def __init__(self, img):
        self.img = img
        (self.magic, self.order, self.n_words, self.n_cls, self.log2, self.bos, self.eos, self.cb) = struct.unpack_from("<8I", img, 0)
        self.uni_off, self.cls_off, self.slot_off, self.n_ngrams = struct.unpack_from("<4Q", img, 32)
        self.edge_off, self.node_off = struct.unpack_from("<2Q", img, 64)
        self.log2_edges, self.n_nodes, self.space, self.n_lex, self.n_drop = struct.unpack_from("<5I", img, 80)
        self.uni = np.frombuffer(img, np.float32, 2 * self.n_words, self.uni_off).reshape(-1, 2)
        n_edges = 1 << self.log2_edges
        e = np.frombuffer(img, np.uint64, 2 * n_edges, self.edge_off).reshape(-1, 2)
        self.edge_key = e[:, 0]
        self.edge_child = (e[:, 1] & np.uint64(0xffffffff)).astype(np.int64)
        self.node_word = np.frombuffer(img, np.int32, self.n_nodes, self.node_off)
        self.longest_chain = 0

    def child(self, node, c):
        key, mask = (node << 32) | c, (1 << self.log2_edges) - 1
        at, steps = _mix(key) & mask, 1
        while True:
            assert steps <= mask + 1, "the probe went round the table"
            k = int(self.edge_key[at])
            if k == key:
                self.longest_chain = max(self.longest_chain, steps)
                return int(self.edge_child[at])
            if k == EMPTY:
                return -1
            at, steps = (at + 1) & mask, steps + 1

    def probe(self, g, w):
        key, mask = (g << 32) | w, (1 << self.log2) - 1
        at = _mix(key) & mask
        while True:
            k, lp, bw = struct.unpack_from("<Qff", self.img, self.slot_off + 16 * at)
            if k == key:
                return self.n_words + at, lp, bw
            if k == EMPTY:
                return None
            at = (at + 1) & mask

    def cond_log10(self, ctx, c):
        """log10 p(c | ctx), ctx nearest first, LM word ids: the kernel's two chains"""
        bows = []
        if ctx:
            g = ctx[0]
            bows.append(float(self.uni[g, 1]))
            for w in ctx[1:]:
                r = self.probe(g, w)
                if r is None:
                    break
                g = r[0]
                bows.append(r[2])
        g, lp, m = c, float(self.uni[c, 0]), 0
        for d, w in enumerate(ctx):
            r = self.probe(g, w)
            if r is None:
                break
            g, lp, m = r[0], r[1], d + 1
        return lp + sum(bows[m:])


def check_against_trie(im: Image, wl: WO.WordLm, n_cls: int):
    """every (node, class) edge and every node -> word id of the image equals the Python trie; returns word -> LM word id"""
    ids, edges, nodes = {}, 0, 0
    stack = [(wl.trie, 0)]
    seen = set()
    while stack:
        node, at = stack.pop()
        assert at not in seen and 0 <= at < im.n_nodes
        seen.add(at)
        nodes += 1
        w = int(im.node_word[at])
        if WO.WORD in node:
            assert 0 <= w < im.n_words and node[WO.WORD] not in ids
            ids[node[WO.WORD]] = w
        else:
            assert w == -1
        for c in range(n_cls):
            ch = im.child(at, c)
            if c in node:
                assert ch > 0, (at, c)
                edges += 1
                stack.append((node[c], ch))
            else:
                assert ch == -1, (at, c)
    assert nodes == im.n_nodes
    used = int((im.edge_key != np.uint64(EMPTY)).sum())
    assert used == edges and 2 * used <= len(im.edge_key)          # nothing but the trie's edges; load <= 1/2
    assert len(set(ids.values())) == len(ids)
    return ids


@pytest.mark.parametrize("order", [1, 3])
def test_word_image_equals_python_trie_and_oracle_scores(tmp_path, order):
    path = S.write_arpa(tmp_path / "w.arpa", WORDS, order, 300, seed=order)
    lm = LO.ArpaOracle.from_file(path)
    assert ("ax",) in lm.ngrams and (order == 1 or any("ax" in g for g in lm.ngrams if len(g) > 1))
    rc, h, msg = _load_words(path, VOCAB, 0)
    assert rc == 0, msg
    o, cb, n_ngrams, (n_lex, n_nodes, n_drop), img = _image(h)
    wl = WO.WordLm(lm, VOCAB)
    assert o == order and cb == 0
    assert n_lex == len(WORDS) - 1 == len(wl.words) and n_drop == 1 and wl.dropped == ["ax"]
    im = Image(img)
    assert im.magic == WORD_MAGIC and im.space == 0 and (im.n_lex, im.n_drop, im.n_nodes) == (n_lex, n_drop, n_nodes)
    assert im.n_words == n_lex + 2                                    # the spellable words, <s> and </s>
    ids = check_against_trie(im, wl, len(VOCAB) + 1)
    assert sorted(ids) == sorted(WORDS[:-1])
    ids["<s>"], ids["</s>"] = im.bos, im.eos
    keep = set(ids)
    kept = [g for g in lm.ngrams if all(w in keep for w in g)]
    assert n_ngrams == len(kept) < len(lm.ngrams)                     # every n-gram with "ax" is left out
    rng = np.random.default_rng(0)
    grams = [g for g in kept if len(g) == order][:200]
    grams += [tuple(rng.choice(WORDS[:-1], order)) for _ in range(200)]  # mostly unseen: backed off
    for g in grams:
        got = im.cond_log10([ids[w] for w in reversed(g[:-1])], ids[g[-1]])
        assert got == pytest.approx(lm.cond_log10(g), abs=1e-5), g


def test_word_image_of_20000_random_words(tmp_path):
    letters = ["'"] + [chr(ord("a") + i) for i in range(26)]
    vocab = [" "] + letters
    words = WS.random_words(20000, letters, 7)
    sents = [words[i:i + 10] for i in range(0, len(words), 10)]
    path = tmp_path / "big.arpa"
    path.write_text(S.arpa_text(sents, 2))
    rc, h, msg = _load_words(path, vocab, 0)
    assert rc == 0, msg
    _, cb, _, (n_lex, n_nodes, n_drop), img = _image(h)
    assert cb == 0 and n_lex == 20000 and n_drop == 0
    lm = LO.ArpaOracle.from_file(path)
    wl = WO.WordLm(lm, vocab)
    im = Image(img)
    ids = check_against_trie(im, wl, len(vocab) + 1)
    assert len(ids) == 20000 and n_nodes > 20000
    assert im.longest_chain > 1                                       # probe chains did occur
    ids["<s>"], ids["</s>"] = im.bos, im.eos
    for g in [g for g in lm.ngrams if len(g) == 2][:300]:
        assert im.cond_log10([ids[g[0]]], ids[g[1]]) == pytest.approx(lm.cond_log10(g), abs=1e-5)


def test_load_arpa_picks_the_mode(tmp_path):
    from lightning_asr_amd import ops
    from lightning_asr_amd.beam_search import BeamSearchDecoderWithLM
    w = S.write_arpa(tmp_path / "w.arpa", WORDS, 2, 200, seed=1)
    lm = ops.load_arpa(w, VOCAB, "cpu", alpha=0.5, beta=2.0)            # the parent commit raises NotImplementedError here
    assert not lm.is_character_based() and lm.order == 2 and (lm.alpha, lm.beta) == (0.5, 2.0)
    assert lm.n_lexicon_words == len(WORDS) - 1 and lm.n_dropped_words == 1
    assert lm.image.dtype == torch.uint8 and struct.unpack_from("<I", lm.image.numpy().tobytes(), 0)[0] == WORD_MAGIC
    with pytest.raises(NotImplementedError, match="word-level"):
        ops.load_arpa(w, ["a", "b", "c", "d"], "cpu")                  # no space label
    with pytest.raises(NotImplementedError, match="word-level"):
        ops.load_arpa(w, [" ", "a", "b", " ", "c", "d"], "cpu")        # two of them
    c = S.write_arpa(tmp_path / "c.arpa", ["a", "b", "c", "d"], 3, 100, seed=2)
    for vocab in (["a", "b", "c", "d"], VOCAB):                         # a character ARPA loads as before, space or not
        cl = ops.load_arpa(c, vocab, "cpu")
        assert cl.is_character_based() and cl.order == 3 and cl.n_lexicon_words == 0
        assert struct.unpack_from("<I", cl.image.numpy().tobytes(), 0)[0] == CHAR_MAGIC
    with pytest.raises(ValueError):
        ops.ctc_beam_decode_lm(torch.zeros(1, 4, 5), None, 4, lm)      # 4 classes + blank; the LM was loaded for 5 labels
    with pytest.raises(ValueError):
        ops.ctc_beam_decode_lm(torch.zeros(1, 4, 6), None, 5, lm, beam_width=129)
    bad = tmp_path / "bad.arpa"
    bad.write_text(open(w).read().replace("\\end\\", ""))
    with pytest.raises(ValueError, match="line"):
        ops.load_arpa(bad, VOCAB, "cpu")
    dec = BeamSearchDecoderWithLM(VOCAB, 8, 0.5, 2.0, w, 4, device="cpu")
    assert not dec.scorer.is_character_based()


def test_c_abi_argument_errors_without_a_gpu(tmp_path):
    lib = _lib()
    w = S.write_arpa(tmp_path / "w.arpa", WORDS, 2, 100, seed=1)
    c = S.write_arpa(tmp_path / "c.arpa", ["a", "b", "c", "d"], 2, 100, seed=2)
    assert lib.lasr_arpa_load_words(None, None, 0, 0, ctypes.byref(ctypes.c_void_p())) == -1
    for sid in (-1, 1, 5):                                             # outside the vocabulary, or not the space
        rc, h, msg = _load_words(w, VOCAB, sid)
        assert rc == -5 and "space_id" in msg and not h.value, (sid, rc, msg)
    rc, h, msg = _load_words(w, [" ", "a", " "], 0)
    assert rc == -5 and not h.value                                    # two space labels
    rc, h, msg = _load_words(c, VOCAB, 0)
    assert rc == -5 and "character-level" in msg and not h.value
    rc, h, msg = _load_words(tmp_path / "nope.arpa", VOCAB, 0)
    assert rc == -6 and "cannot open" in msg
    bad = tmp_path / "bad.arpa"
    bad.write_text(open(w).read().replace("ngram 2=", "ngram 2=9"))
    rc, h, msg = _load_words(bad, VOCAB, 0)
    assert rc == -4 and "line" in msg and "declares" in msg
    b = tmp_path / "lm.bin"
    b.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\x00")
    rc, h, msg = _load_words(b, VOCAB, 0)
    assert rc == -5 and "binary" in msg
    # lasr_arpa_lexicon_info: only for a handle of lasr_arpa_load_words
    assert lib.lasr_arpa_lexicon_info(None, None, None, None) == -1
    arr = (ctypes.c_char_p * 2)(b"a", b"b")
    h = ctypes.c_void_p()
    assert lib.lasr_arpa_load(str(c).encode(), ctypes.cast(arr, ctypes.c_void_p), 2, ctypes.byref(h)) == 0
    assert lib.lasr_arpa_lexicon_info(h, None, None, None) == -1
    lib.lasr_arpa_free(h)

    fake = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails its checks first

    def call(**kw):
        a = dict(logp=fake, img=fake, W=16, n_best=1, alpha=1.0, beta=1.0, nb=1 << 20, blank=28)
        a.update(kw)
        return lib.lasr_ctc_beam_decode_wlm(a["logp"], None, 2, 10, 29, a["blank"], a["W"], 40, 1.0, a["n_best"], a["img"],
                                            a["alpha"], a["beta"], fake, fake, fake, fake, fake, a["nb"], None)
    assert call(img=None) == -1 and b"lasr_ctc_beam_decode_wlm: null pointer" in lib.lasr_last_error()
    assert call(logp=None) == -1
    assert call(n_best=17) == -1
    assert call(alpha=float("nan")) == -1 and call(beta=float("inf")) == -1
    assert call(blank=29) == -1
    assert call(W=129, n_best=1) == -2
    assert call(nb=16) == -3


def test_oracle_unbounded_beam_equals_brute_force_with_lexicon():
    vocab = [" ", "a", "b"]
    words = ["a", "ab", "ba", "bb"]
    wl = WO.WordLm(LO.ArpaOracle(S.arpa_text(S.sentences(words, 40, 1), 2)), vocab)
    assert sorted(wl.words) == words
    rng = np.random.default_rng(0)
    for alpha, beta in [(0.5, 1.0), (1.0, -0.5), (0.0, 0.3)]:
        for _ in range(4):
            T, C = 5, 4
            x = torch.log_softmax(torch.tensor(rng.normal(size=(T, C)) * 1.5), -1).numpy()
            exact = O.brute_force(x, C - 1)
            hyps, _, fired, rejected, _ = WO.beam_search(x, T, C - 1, wl, alpha, beta, 10 ** 6, C, 1.0, 10 ** 4)
            assert fired == 0 and rejected > 0
            want = {p: s + wl.bonus(p, alpha, beta) + wl.end_term(p, alpha, beta) for p, s in exact.items() if wl.exists(p)}
            assert () in want and (0,) not in want and (1, 0, 0) not in want and (2,) in want and (2, 0) not in want
            assert {p for p, _, _ in hyps} == set(want)
            assert [f for _, f, _ in hyps] == sorted((f for _, f, _ in hyps), reverse=True)
            for p, f, am in hyps:
                assert f == pytest.approx(want[p], abs=1e-9)
                assert am == pytest.approx(exact[p], abs=1e-9)
    # an unfinished word that is no word carries OOV_SCORE; one that is a word carries its LM term
    assert wl.end_term((2,), 0.5, 1.0) == 0.5 * LO.OOV_SCORE + 1.0
    assert wl.end_term((1, 2), 0.5, 1.0) == pytest.approx(0.5 * wl.lm.emission(["ab"]) + 1.0)
    assert wl.end_term((1, 0), 0.5, 1.0) == 0.0 and wl.end_term((), 0.5, 1.0) == 0.0
