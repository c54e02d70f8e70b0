"""CPU tier of the LM-fused CTC prefix beam search: the f64 oracle (tests/helpers/ctc_beam_lm_oracle.py) against hand-computed
ARPA backoff, brute-force path enumeration and the LM-free oracle; the ARPA reader behind lasr_arpa_load / _info / _write_image
on good files and every reject case; and the Python surface's exceptions.  No GPU."""
import ctypes
import math
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

LOGE = LO.NUM_FLT_LOGE

SMALL = """
\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-99\t<s>\t-0.3
-0.7\t</s>
-0.5\ta\t-0.2
-0.6\tb\t-0.25
-1.0\t<unk>

\\2-grams:
-0.4\t<s> a\t-0.1
-0.3\ta b\t-0.15
-0.35\tb a\t-0.05
-0.2\tb </s>

\\3-grams:
-0.1\t<s> a b
-0.12\ta b a

\\end\\
"""


def test_oracle_scorer_hand_computed():
    lm = LO.ArpaOracle(SMALL)
    assert lm.order == 3 and lm.vocab == {"<s>", "</s>", "a", "b"}
    # (<s> <s> a): "<s> <s> a" and context "<s> <s>" not stored; "<s> a" stored
    assert lm.emission(["a"]) == pytest.approx(-0.4 / LOGE)
    # (<s> a b): stored 3-gram
    assert lm.emission(["a", "b"]) == pytest.approx(-0.1 / LOGE)
    # (a b b): "a b b", "b b" not stored -> p(b) + bow(a b) + bow(b)
    assert lm.emission(["a", "b", "b"]) == pytest.approx((-0.6 - 0.15 - 0.25) / LOGE)
    # (b a a): "b a a", "a a" not stored; bow(b a) = -0.05, bow(a) = -0.2
    assert lm.emission(["x", "b", "a", "a"][1:]) == pytest.approx((-0.5 - 0.05 - 0.2) / LOGE)
    # (<s> <s> b): "<s> b" not stored, context "<s> <s>" not stored, bow(<s>) = -0.3
    assert lm.emission(["b"]) == pytest.approx((-0.6 - 0.3) / LOGE)
    # OOV: in the word itself, in the context, and <unk>
    assert lm.emission(["a", "z"]) == LO.OOV_SCORE
    assert lm.emission(["z", "a"]) == LO.OOV_SCORE
    assert lm.emission(["z", "a", "b", "a"]) == pytest.approx(-0.12 / LOGE)  # the OOV label left the 3-word window
    assert lm.emission(["a", "<unk>"]) == LO.OOV_SCORE
    # sentence: <s> <s> a b </s> -> windows (<s> <s> a), (<s> a b), (a b </s>)
    want = (-0.4 + -0.1 + (-0.2 - 0.15)) / LOGE
    assert lm.sentence(["a", "b"]) == pytest.approx(want)
    # empty: <s> <s> <s> </s> -> (<s> <s> <s>) and (<s> <s> </s>)
    assert lm.sentence([]) == pytest.approx(((-99 - 0.3) + (-0.7 - 0.3)) / LOGE)


def _cases(n=12, seed=0):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        T, C = int(rng.integers(1, 6)), int(rng.integers(3, 5))
        yield torch.log_softmax(torch.tensor(rng.normal(size=(T, C)) * 1.5), -1).numpy()


def test_oracle_unbounded_beam_equals_brute_force_with_lm():
    vocab = ["a", "b", "c"]
    lm = LO.ArpaOracle(S.arpa_text(S.sentences(["a", "b"], 40, 1), 3))       # "c" is OOV
    for alpha, beta in [(0.5, 1.0), (1.0, -0.5), (0.0, 0.3)]:
        for x in _cases():
            T, C = x.shape
            exact = O.brute_force(x, C - 1)
            hyps, _, fired = LO.beam_search(x, T, C - 1, vocab[:C - 1], lm, alpha, beta, 10 ** 6, C, 1.0, 1000)
            assert fired == 0
            fused = {p: s + alpha * sum(lm.emission([vocab[c] for c in p[:i + 1]]) for i in range(len(p))) + beta * len(p)
                     for p, s in exact.items()}
            best = max(fused.items(), key=lambda kv: kv[1])
            assert hyps[0][0] == best[0] and hyps[0][1] == pytest.approx(best[1], abs=1e-9)
            for p, f, am in hyps:
                assert f == pytest.approx(fused[p], abs=1e-9)
                assert am == pytest.approx(f - beta * len(p) - alpha * lm.sentence([vocab[c] for c in p]), abs=1e-9)


def test_oracle_without_lm_weight_equals_lm_free_oracle():
    lm = LO.ArpaOracle(SMALL)
    vocab = ["a", "b", "c"]
    for x in _cases(seed=3):
        T, C = x.shape
        for W in (1, 2, 4):
            for cp in (1.0, 0.8):
                want, _ = O.beam_search(x, T, C - 1, W, C, cp, W)
                got, _, _ = LO.beam_search(x, T, C - 1, vocab[:C - 1], lm, 0.0, 0.0, W, C, cp, W, use_filter=False)
                assert [p for p, _, _ in got] == [p for p, _ in want]
                assert all(abs(a[1] - b[1]) < 1e-12 for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------ the ARPA reader (C ABI)
def _lib():
    from lightning_asr_amd import _lib
    return _lib.load()


def _load(path, vocab):
    lib = _lib()
    words = [w.encode() for w in vocab]
    arr = (ctypes.c_char_p * max(len(words), 1))(*words)
    h = ctypes.c_void_p()
    rc = lib.lasr_arpa_load(str(path).encode(), ctypes.cast(arr, ctypes.c_void_p), len(words), ctypes.byref(h))
    return rc, h, lib.lasr_last_error().decode()


def _image(h):
    lib = _lib()
    order, cb, n, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_size_t()
    assert lib.lasr_arpa_info(h, ctypes.byref(order), ctypes.byref(cb), ctypes.byref(n), ctypes.byref(nb)) == 0
    buf = np.zeros(nb.value, dtype=np.uint8)
    assert lib.lasr_arpa_write_image(h, buf.ctypes.data, 16) == -3          # too small
    assert lib.lasr_arpa_write_image(h, buf.ctypes.data, nb.value) == 0
    lib.lasr_arpa_free(h)
    return order.value, cb.value, n.value, buf.tobytes()


def _mix(k):
    M = (1 << 64) - 1
    k = ((k ^ (k >> 30)) * 0xbf58476d1ce4e5b9) & M
    k = ((k ^ (k >> 27)) * 0x94d049bb133111eb) & M
    return k ^ (k >> 31)


def _image_score(img, vocab_ids, ctx_words, c):
    """lm(c | ctx) by walking the image as the kernel does (ctx nearest first, LM word ids)"""
    magic, order, n_words, n_cls, log2, bos, eos, cb = struct.unpack_from("<8I", img, 0)
    uni_off, cls_off, slot_off, _ = struct.unpack_from("<4Q", img, 32)
    uni = np.frombuffer(img, np.float32, 2 * n_words, uni_off).reshape(-1, 2)
    mask = (1 << log2) - 1

    def probe(g, w):
        key = (g << 32) | w
        at = _mix(key) & mask
        while True:
            k, lp, bw = struct.unpack_from("<Qff", img, slot_off + 16 * at)
            if k == key:
                return n_words + at, lp, bw
            if k == (1 << 64) - 1:
                return None
            at = (at + 1) & mask

    ctx = list(ctx_words)
    bows, g = [], None
    # context chain bows
    if ctx:
        g = ctx[0]
        bows.append(float(uni[g, 1]))
        for w in ctx[1:]:
            r = probe(g, w)
            if r is None:
                break
            g = r[0]
            bows.append(r[2])
    g, lp, m = c, float(uni[c, 0]), 0
    for d, w in enumerate(ctx):
        r = probe(g, w)
        if r is None:
            break
        g, lp, m = r[0], r[1], d + 1
    return lp + sum(bows[m:])


def test_arpa_load_good_file_and_image_walk(tmp_path):
    p = tmp_path / "small.arpa"
    p.write_text(SMALL)
    rc, h, msg = _load(p, ["a", "b", "c", "<unk>"])
    assert rc == 0, msg
    order, cb, n, img = _image(h)
    assert order == 3 and cb == 1
    assert n == 4 + 4 + 2                          # <s> </s> a b + every 2- and 3-gram (all over mapped words)
    magic, _, n_words, n_cls, _, bos, eos, _ = struct.unpack_from("<8I", img, 0)
    assert magic == 0x4d4c5341 and n_words == 4 and n_cls == 4
    cls = np.frombuffer(img, np.int32, 4, struct.unpack_from("<Q", img, 40)[0])
    assert cls[2] == -1 and cls[3] == -1            # "c" is not in the LM, "<unk>" is OOV by definition
    a, b = int(cls[0]), int(cls[1])
    lm = LO.ArpaOracle(SMALL)
    ids = {"<s>": bos, "a": a, "b": b, "</s>": eos}
    for ng in [("<s>", "<s>", "a"), ("<s>", "a", "b"), ("a", "b", "b"), ("b", "a", "a"), ("<s>", "<s>", "b"), ("a", "b", "a"),
               ("a", "b", "</s>")]:
        got = _image_score(img, ids, [ids[w] for w in reversed(ng[:-1])], ids[ng[-1]])
        assert got == pytest.approx(lm.cond_log10(ng), abs=1e-6), ng


def test_arpa_load_drops_unmapped_words_and_synth_orders(tmp_path):
    labels = list("abcdefgh")
    for order in (1, 2, 3, 6):
        p = S.write_arpa(tmp_path / ("o%d.arpa" % order), labels, order, 200, seed=order)
        rc, h, msg = _load(p, labels)
        assert rc == 0, msg
        o, cb, n_all, _ = _image(h)
        assert o == order and cb == 1
        rc, h, _ = _load(p, labels[:4])
        _, _, n_few, _ = _image(h)
        assert n_few < n_all
    # word-level: loads, reports char_based = 0
    p = S.write_arpa(tmp_path / "w.arpa", labels, 2, 50, multichar=True)
    rc, h, _ = _load(p, labels)
    assert rc == 0 and _image(h)[1] == 0
    # no <s>: loads
    p = S.write_arpa(tmp_path / "nobos.arpa", labels, 3, 50, no_bos=True)
    rc, h, _ = _load(p, labels)
    assert rc == 0
    _image(h)


BAD = {
    "count": (SMALL.replace("ngram 2=4", "ngram 2=5"), "declares"),
    "nan": (SMALL.replace("-0.3\ta b", "nan\ta b"), "line 16"),
    "fields": (SMALL.replace("-0.3\ta b\t-0.15", "-0.3\ta b c d"), "line 16"),
    "suffix": (SMALL.replace("-0.3\ta b\t-0.15\n", "").replace("ngram 2=4", "ngram 2=3"), "suffix"),
    "order7": (SMALL.replace("ngram 3=2", "ngram 3=2\nngram 4=1\nngram 5=1\nngram 6=1\nngram 7=1"), "order 7"),
    "no_end": (SMALL.replace("\\end\\", ""), "before \\end\\"),
    "no_data": ("hello\n", "\\data\\"),
    "dup": (SMALL.replace("-0.35\tb a", "-0.35\ta b"), "duplicate"),
    "section": (SMALL.replace("\\3-grams:", "\\4-grams:"), "line"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_arpa_load_rejects(tmp_path, case):
    text, needle = BAD[case]
    p = tmp_path / (case + ".arpa")
    p.write_text(text)
    rc, h, msg = _load(p, ["a", "b"])
    assert rc == -4, (rc, msg)                      # LASR_E_FORMAT
    assert needle in msg, msg
    assert not h.value


def test_arpa_load_rejects_binary_missing_and_suffix_incomplete_synth(tmp_path):
    p = tmp_path / "lm.bin"
    p.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\x00\x01\x02")
    rc, h, msg = _load(p, ["a"])
    assert rc == -5 and "binary" in msg             # LASR_E_UNSUPPORTED
    rc, h, msg = _load(tmp_path / "nope.arpa", ["a"])
    assert rc == -6 and "cannot open" in msg                     # LASR_E_IO
    rc, h, msg = _load(tmp_path, ["a"])                           # a directory opens but cannot be read
    assert rc == -6 and "cannot" in msg
    p = S.write_arpa(tmp_path / "si.arpa", list("abcd"), 3, 100, suffix_incomplete=True)
    rc, h, msg = _load(p, list("abcd"))
    assert rc == -4 and "suffix" in msg and "line" in msg
    lib = _lib()
    assert lib.lasr_arpa_load(None, None, 0, ctypes.byref(ctypes.c_void_p())) == -1
    assert lib.lasr_arpa_info(None, None, None, None, None) == -1
    p = tmp_path / "small.arpa"
    p.write_text(SMALL)
    h = ctypes.c_void_p()
    assert lib.lasr_arpa_load(str(p).encode(), None, 0, ctypes.byref(h)) == 0   # no labels: an image with <s> / </s> only
    assert _image(h)[2] == 2 + 0


def test_beam_lm_workspace_and_arguments_without_a_gpu():
    lib = _lib()
    assert lib.lasr_ctc_beam_lm_workspace_bytes(2, 10, 28, 16, 40) == lib.lasr_ctc_beam_workspace_bytes(2, 10, 28, 16, 40)
    assert lib.lasr_ctc_beam_lm_workspace_bytes(2, 10, 28, 129, 40) == 0
    fake = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails its checks first

    def call(**kw):
        a = dict(logp=fake, img=fake, W=16, n_best=1, alpha=1.0, beta=1.0, nb=1 << 20, blank=27)
        a.update(kw)
        return lib.lasr_ctc_beam_decode_lm(a["logp"], None, 2, 10, 28, a["blank"], a["W"], 40, 1.0, a["n_best"], a["img"],
                                           a["alpha"], a["beta"], fake, fake, fake, fake, fake, a["nb"], None)
    assert call(img=None) == -1 and b"null pointer" in lib.lasr_last_error()
    assert call(logp=None) == -1
    assert call(n_best=17) == -1
    assert call(alpha=float("nan")) == -1 and call(beta=float("inf")) == -1
    assert call(blank=28) == -1
    assert call(W=129, n_best=1) == -2
    assert call(nb=16) == -3


def test_python_surface_exceptions(tmp_path):
    from lightning_asr_amd import ops
    from lightning_asr_amd.beam_search import BeamSearchDecoderWithLM
    with pytest.raises(FileNotFoundError):
        ops.load_arpa(tmp_path / "missing.arpa", ["a"], "cpu")
    with pytest.raises(NotImplementedError):
        BeamSearchDecoderWithLM(["a", "b"], 8, 1.0, 1.0, str(tmp_path / "missing.arpa"), 4)
    b = tmp_path / "lm.bin"
    b.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\x00")
    with pytest.raises(NotImplementedError):
        ops.load_arpa(b, ["a"], "cpu")
    w = S.write_arpa(tmp_path / "w.arpa", list("abc"), 2, 30, multichar=True)
    with pytest.raises(NotImplementedError, match="word-level"):
        ops.load_arpa(w, list("abc"), "cpu")
    bad = tmp_path / "bad.arpa"
    bad.write_text(SMALL.replace("ngram 2=4", "ngram 2=5"))
    with pytest.raises(ValueError, match="line"):
        BeamSearchDecoderWithLM(["a", "b"], 8, 1.0, 1.0, str(bad), 4, device="cpu")
    ok = tmp_path / "ok.arpa"
    ok.write_text(SMALL)
    lm = ops.load_arpa(ok, ["a", "b"], "cpu", alpha=0.5, beta=2.0)
    assert lm.order == 3 and lm.is_character_based() and lm.alpha == 0.5 and lm.beta == 2.0
    assert lm.image.dtype == torch.uint8 and lm.image.device.type == "cpu"
    dec = BeamSearchDecoderWithLM(["a", "b"], 8, 0.5, 2.0, str(ok), 4, device="cpu")
    assert dec.scorer.order == 3
    x = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode_lm(x, None, 2, lm, beam_width=129)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode_lm(x, None, 2, lm, beam_width=4, n_best=5)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode_lm(torch.zeros(1, 4, 5), None, 4, lm)          # 4 labels, the LM was loaded for 2
    with pytest.raises(ValueError):
        ops.ctc_beam_decode_lm(x, None, 2, lm, alpha=math.inf)
    with pytest.raises(TypeError):
        ops.ctc_beam_decode_lm(x, None, 2, None)
