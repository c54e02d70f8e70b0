"""GPU tier of the CTC prefix beam search fused with a word-level LM and its lexicon (csrc/ctc_beam.hip,
lasr_ctc_beam_decode_wlm): n-best lists against the f64 oracle (tests/helpers/ctc_beam_wlm_oracle.py) over synthetic word
ARPA files (arpa_synth.write_arpa with words as its labels) and log-probs peaky around sentences of those words
(tests/helpers/wlm_synth.py); the end-of-utterance re-rank, the early cutoff, ragged lengths, the widest candidate set, a
longer batch, determinism, graph capture, images of the wrong kind, and the Python surface.

As in test_gpu_ctc_beam_lm.py, every oracle comparison first asserts that the oracle's decision margin (here including the
gaps of the final re-rank) clears margin_min(T); scores must agree to that relative tolerance.  Every case also asserts, on
the oracle, that the lexicon rejected candidates and that the best hypothesis holds at least two spaces."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import arpa_synth as S  # noqa: E402
import ctc_beam_wlm_oracle as WO  # noqa: E402
import wlm_synth as WS  # noqa: E402

pytestmark = pytest.mark.gpu

VOCAB = [" ", "a", "b", "c", "d"]                                  # C = 6 with the blank
WORDS = ["a", "ab", "abc", "aa", "abba", "b", "bad", "cab", "dad", "add", "cad", "dab", "ax"]     # "ax" cannot be spelled
EN_SP = [" ", "'"] + [chr(ord("a") + i) for i in range(26)]       # predict.EN_LABELS, C = 29
_cache = {}


def margin_min(T: int) -> float:
    return 8.0 * 2.0 ** -24 * math.sqrt(max(int(T), 1))            # test_gpu_ctc_beam_lm.margin_min


def word_lm(path, vocab):
    key = (str(path), len(vocab))
    if key not in _cache:
        _cache[key] = WO.WordLm.from_file(path, vocab)
    return _cache[key]


def wlm_case(vocab, words, path, B, T, W, k, cp, n_best, alpha, beta, lens=None, seeds=tuple(range(32)), want=None, **gen):
    """the first seed whose oracle margin clears margin_min(T) (and that `want`(oracle result) accepts):
    (log-probs, hypotheses, early-cutoff drops, lexicon rejections, reranked)"""
    wl = word_lm(path, vocab)
    worst = 0.0
    for seed in seeds:
        x, _ = WS.sentence_logp(vocab, words, B, T, seed, **gen)
        out = WO.beam_search_batch(x.numpy(), lens, len(vocab), wl, alpha, beta, W, k, cp, n_best)
        if out[1] >= margin_min(T) and (want is None or want(x, out)):
            return (x,) + out[:1] + out[2:]
        worst = max(worst, out[1])
    raise AssertionError("no seed of %s gives an oracle margin above %.2e (best %.2e)" % (seeds, margin_min(T), worst))


def run(dev, x, lens, vocab, path, W, k, cp, n_best, alpha, beta):
    from lightning_asr_amd import ops
    lm = ops.load_arpa(path, vocab, dev, alpha, beta)
    assert not lm.is_character_based()
    lt = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    out = ops.ctc_beam_decode_lm(x.to(dev).contiguous(), lt, len(vocab), lm, W, k, cp, n_best)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def assert_matches(got, res, n_best, T):
    tok, n, sc, am = got
    tol = margin_min(T)
    for b, hyps in enumerate(res):
        for j in range(n_best):
            if j < len(hyps):
                want, fused, acoustic = hyps[j]
                assert n[b, j] == len(want), (b, j, n[b, j], len(want))
                assert tuple(int(c) for c in tok[b, j, :n[b, j]]) == want, (b, j)
                assert (tok[b, j, n[b, j]:] == -1).all()
                assert abs(sc[b, j] - fused) <= tol * max(1.0, abs(fused)), (b, j, float(sc[b, j]), fused)
                assert abs(am[b, j] - acoustic) <= tol * max(1.0, abs(acoustic), abs(fused)), (b, j, float(am[b, j]), acoustic)
            else:
                assert n[b, j] == -1 and sc[b, j] == -np.inf and am[b, j] == -np.inf and (tok[b, j] == -1).all(), (b, j)


def scores_words(res, space=0):
    """every utterance's best hypothesis holds at least two spaces: words were scored during the search"""
    return all(len(hyps) > 0 and sum(c == space for c in hyps[0][0]) >= 2 for hyps in res)


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    d = tmp_path_factory.mktemp("wlm")
    return {o: S.write_arpa(d / ("w%d.arpa" % o), WORDS, o, 400, seed=o) for o in (1, 2, 3, 6)}


@pytest.fixture(scope="module")
def en_lm(tmp_path_factory):
    """a 3-gram over 2 000 random words of the English letters"""
    words = WS.random_words(2000, EN_SP[1:], 11, 1, 7)
    path = tmp_path_factory.mktemp("wlm_en") / "en2000.arpa"
    sents = [words[i:i + 8] for i in range(0, len(words), 8)] + S.sentences(words, 1500, 4)
    path.write_text(S.arpa_text(sents, 3), encoding="utf-8")
    return words, str(path)


# (order, W, k, cutoff_prob, alpha, beta): orders 1, 2, 3, 6; widths 1, 4, 16, 128; cutoff_top_n 6 and 3; cutoff_prob 1.0 and
# 0.95; beta zero, positive and negative; alpha 0 (the lexicon alone)
CASES = [(1, 16, 6, 1.0, 0.5, 0.0), (2, 1, 6, 1.0, 1.0, 1.0), (2, 4, 6, 1.0, 0.5, -0.5), (3, 16, 6, 1.0, 1.0, 2.0),
         (3, 128, 6, 0.95, 0.8, 1.0), (3, 4, 3, 1.0, 0.5, 0.5), (6, 16, 6, 1.0, 1.0, 1.5), (6, 128, 6, 1.0, 0.3, -1.0),
         (1, 128, 3, 0.95, 1.0, 2.5), (6, 4, 3, 0.95, 2.0, 0.0), (3, 16, 6, 1.0, 0.0, 0.0), (2, 16, 6, 1.0, 0.0, 1.0)]


HOT_CP = 4.0


@pytest.mark.parametrize("order,W,k,cp,alpha,beta", CASES)
def test_beam_wlm_matches_oracle(dev, lms, order, W, k, cp, alpha, beta):
    B, T = 2, 48
    n_best = min(W, 4)
    # with cutoff_prob < 1 a hot class of 8 would be the only class kept, and one corrupted frame would end the beam
    gen = {"hot": HOT_CP} if cp < 1.0 else {}
    x, res, _, rejected, _ = wlm_case(VOCAB, WORDS[:-1], lms[order], B, T, W, k, cp, n_best, alpha, beta,
                                      want=lambda x, out: scores_words(out[0]), **gen)
    assert rejected > 0 and scores_words(res)
    assert_matches(run(dev, x, None, VOCAB, lms[order], W, k, cp, n_best, alpha, beta), res, n_best, T)


def test_beam_wlm_end_term_reranks(dev, lms):
    """the end-of-utterance term changes the order of the returned entries: the oracle without it ranks other hypotheses (or
    another order); the kernel matches the oracle with it"""
    B, T, W, alpha, beta, n_best = 2, 48, 16, 1.0, 1.0, 4
    path = lms[3]
    x, res, _, rejected, reranked = wlm_case(VOCAB, WORDS[:-1], path, B, T, W, 6, 1.0, n_best, alpha, beta,
                                             want=lambda x, out: out[4] and scores_words(out[0]))
    assert reranked and rejected > 0 and scores_words(res)
    plain = WO.beam_search_batch(x.numpy(), None, len(VOCAB), word_lm(path, VOCAB), alpha, beta, W, 6, 1.0, n_best, end_term=False)[0]
    assert [[p for p, _, _ in h] for h in plain] != [[p for p, _, _ in h] for h in res]
    assert_matches(run(dev, x, None, VOCAB, path, W, 6, 1.0, n_best, alpha, beta), res, n_best, T)


def test_beam_wlm_early_cutoff_decides(dev, lms):
    """beta = 2.5 on a full beam: the oracle without the early cutoff returns other scores (or hypotheses); the kernel matches
    the oracle with it"""
    B, T, W, alpha, beta = 2, 48, 16, 0.5, 2.5
    path = lms[3]
    wl = word_lm(path, VOCAB)

    def decides(x, out):
        nf = WO.beam_search_batch(x.numpy(), None, len(VOCAB), wl, alpha, beta, W, 6, 1.0, 4, use_filter=False)[0]
        return out[2] > 0 and scores_words(out[0]) and any(
            a[0] != b[0] or abs(a[1] - b[1]) > 100 * margin_min(T) * max(1.0, abs(a[1])) for ra, rb in zip(out[0], nf) for a, b in zip(ra, rb))
    x, res, fired, rejected, _ = wlm_case(VOCAB, WORDS[:-1], path, B, T, W, 6, 1.0, 4, alpha, beta, want=decides)
    assert fired > 0 and rejected > 0 and scores_words(res)
    assert_matches(run(dev, x, None, VOCAB, path, W, 6, 1.0, 4, alpha, beta), res, 4, T)


def test_beam_wlm_ragged_lengths_and_unfinished_word(dev, lms):
    B, T, W, alpha, beta = 6, 48, 16, 1.0, 1.0
    lens = [48, 0, 1, 17, 33, 2]
    path = lms[3]
    wl = word_lm(path, VOCAB)

    def unfinished(x, out):
        # some utterance's best hypothesis ends inside a word that is no word: it carries the OOV_SCORE term
        return scores_words(out[0][:1]) and any(
            h[0][0] and h[0][0][-1] != 0 and wl.end_term(h[0][0], alpha, beta) == alpha * WO.OOV_SCORE + beta for h in out[0])
    x, res, _, rejected, _ = wlm_case(VOCAB, WORDS[:-1], path, B, T, W, 6, 1.0, 3, alpha, beta, lens=lens, want=unfinished,
                                      seeds=tuple(range(64)))
    assert rejected > 0
    oov = [b for b, h in enumerate(res) if h[0][0] and wl.end_term(h[0][0], alpha, beta) == alpha * WO.OOV_SCORE + beta]
    assert oov
    got = run(dev, x, lens, VOCAB, path, W, 6, 1.0, 3, alpha, beta)
    assert_matches(got, res, 3, T)
    assert got[1][1, 0] == 0 and got[2][1, 0] == 0.0 and got[3][1, 0] == 0.0    # lens 0: the empty hypothesis, score 0
    for b in oov:
        assert got[2][b, 0] - got[3][b, 0] < 0.5 * alpha * WO.OOV_SCORE      # the -1000 is in the fused score, not the acoustic


def test_beam_wlm_widest_candidate_set(dev, en_lm):
    """C = 29 (EN_LABELS), a 2 000-word lexicon, beam 128, cutoff_top_n 29: 128 * 30 candidates per frame, the widest J the
    dispatcher picks for this vocabulary"""
    words, path = en_lm
    B, T, W, k = 2, 48, 128, 29
    x, res, _, rejected, _ = wlm_case(EN_SP, words, path, B, T, W, k, 1.0, 8, 0.7, 1.0, seeds=tuple(range(8)), hot=10.0, n_words=(4, 10),
                                      want=lambda x, out: scores_words(out[0]))
    assert rejected > 0 and scores_words(res)
    assert_matches(run(dev, x, None, EN_SP, path, W, k, 1.0, 8, 0.7, 1.0), res, 8, T)


SYM47 = EN_SP + [chr(ord("A") + i) for i in range(19)]            # 47 labels: C = 48, the smallest with 41 classes to keep


@pytest.fixture(scope="module")
def sym47_lm(tmp_path_factory):
    """a 3-gram over 2 000 random words of SYM47's 46 letters"""
    words = WS.random_words(2000, SYM47[1:], 13, 1, 7)
    path = tmp_path_factory.mktemp("wlm_sym47") / "sym2000.arpa"
    sents = [words[i:i + 8] for i in range(0, len(words), 8)] + S.sentences(words, 1500, 5)
    path.write_text(S.arpa_text(sents, 3), encoding="utf-8")
    return words, str(path)


# The rungs of the candidate ladder the cases above leave out (they run 1, 2, 4 and 16 candidates per thread): C = 29 at beam 64
# has 64 * 30 candidates, J = 8; C = 48 keeps cutoff_top_n = 40 labels, and beam 128 then has 128 * 41, J = 33.
@pytest.mark.parametrize("wide,W", [(False, 64), (True, 128)], ids=["J8", "J33"])
def test_beam_wlm_every_other_rung(dev, en_lm, sym47_lm, wide, W):
    vocab, (words, path) = (SYM47, sym47_lm) if wide else (EN_SP, en_lm)
    B, T, k = 2, 30, 40
    x, res, _, rejected, _ = wlm_case(vocab, words, path, B, T, W, k, 1.0, 4, 0.7, 1.0, seeds=tuple(range(8)), hot=10.0, n_words=(3, 6),
                                      want=lambda x, out: scores_words(out[0]))
    assert rejected > 0 and scores_words(res)
    assert_matches(run(dev, x, None, vocab, path, W, k, 1.0, 4, 0.7, 1.0), res, 4, T)


LONG_SEED = 1


def test_beam_wlm_long_batch(dev, en_lm):
    """one B = 8, T = 200 batch: each utterance is held to the oracle where its own margin clears margin_min(T); at least 6 of
    the 8 must (the seed is chosen so that the oracle alone meets that: 7 do)"""
    words, path = en_lm
    B, T, W = 8, 200, 8
    wl = word_lm(path, EN_SP)
    lens = [T] + [int(v) for v in np.random.default_rng(2).integers(120, T + 1, B - 1)]
    x, _ = WS.sentence_logp(EN_SP, words, B, T, LONG_SEED, hot=12.0, n_words=(8, 12))
    got = run(dev, x, lens, EN_SP, path, W, 29, 1.0, 2, 0.5, 1.0)
    ok = 0
    for b in range(B):
        hyps, m, _, rejected, _ = WO.beam_search(x[b].numpy(), lens[b], len(EN_SP), wl, 0.5, 1.0, W, 29, 1.0, 2)
        assert rejected > 0
        if m >= margin_min(T):
            ok += 1
            assert sum(c == 0 for c in hyps[0][0]) >= 2
            assert_matches([g[b:b + 1] for g in got], [hyps], 2, T)
    assert ok >= 6, ok


def test_beam_wlm_deterministic_graph_capture_and_lm_applied(dev, lms):
    from lightning_asr_amd import ops
    B, T, C = 8, 200, 6
    x, _ = WS.sentence_logp(VOCAB, WORDS[:-1], B, T, 5)
    x = x.to(dev).contiguous()
    lens = torch.tensor([200, 150, 1, 0, 199, 77, 120, 200], dtype=torch.int32, device=dev)
    lm = ops.load_arpa(lms[6], VOCAB, dev, 0.8, 1.0)
    a = ops.ctc_beam_decode_lm(x, lens, C - 1, lm, 32, 6, 0.95, 8)
    b = ops.ctc_beam_decode_lm(x, lens, C - 1, lm, 32, 6, 0.95, 8)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.ctc_beam_decode_lm(x, lens, C - 1, lm, 32, 6, 0.95, 8)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = ops.ctc_beam_decode_lm(x, lens, C - 1, lm, 32, 6, 0.95, 8)
    g.replay()
    torch.cuda.synchronize()
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    # the LM-free search is a different result on the same inputs (the lexicon and the LM are applied)
    t0, _, _ = ops.ctc_beam_decode(x, lens, C - 1, 32, 6, 0.95, 8)
    assert not torch.equal(t0, a[0])


def test_image_of_the_other_kind_gives_empty_slots(dev, lms, tmp_path):
    from lightning_asr_amd import _lib, ops
    from lightning_asr_amd.ops import _p, _stream, _ws
    B, T, C, W = 2, 20, 6, 4
    x, _ = WS.sentence_logp(VOCAB, WORDS[:-1], B, T, 1)
    x = x.to(dev).contiguous()
    word = ops.load_arpa(lms[2], VOCAB, dev)
    char = ops.load_arpa(S.write_arpa(tmp_path / "c.arpa", VOCAB[1:], 2, 100, seed=2), VOCAB, dev)
    assert char.is_character_based() and not word.is_character_based()
    nb = int(_lib.load().lasr_ctc_beam_lm_workspace_bytes(B, T, C, W, 6))
    for entry, lm in (("lasr_ctc_beam_decode_wlm", char), ("lasr_ctc_beam_decode_lm", word)):
        tokens, n, scores = ops._beam_outputs(x, 2)
        am = torch.empty_like(scores)
        ws = _ws(nb, x.device)
        _lib.call(entry, _p(x), None, B, T, C, C - 1, W, 6, 1.0, 2, _p(lm.image), 1.0, 1.0, _p(tokens), _p(n), _p(scores), _p(am),
                  _p(ws), nb, _stream())
        torch.cuda.synchronize()
        assert (n == -1).all() and (tokens == -1).all() and torch.isneginf(scores).all() and torch.isneginf(am).all(), entry


# ------------------------------------------------------------------------------------------------ Python surface
def test_decoder_with_word_lm_path(dev, en_lm):
    from lightning_asr_amd.beam_search import BeamSearchDecoderWithLM
    words, path = en_lm
    lens = [60, 45, 12]
    x, res, _, rejected, _ = wlm_case(EN_SP, words, path, 3, 60, 16, 29, 1.0, 3, 1.0, 1.0, lens=lens, hot=10.0, n_words=(4, 10),
                                      want=lambda x, out: scores_words(out[0][:2]))
    assert rejected > 0
    dec = BeamSearchDecoderWithLM(EN_SP, 16, 1.0, 1.0, path, 4, cutoff_prob=1.0, cutoff_top_n=29)
    assert dec.scorer.order == 3 and not dec.scorer.is_character_based() and dec.scorer.n_lexicon_words == 2000
    want = ["".join(EN_SP[c] for c in r[0][0]) for r in res]
    assert dec.forward(x.numpy(), np.array(lens)) == want
    assert dec(x.to(dev), torch.tensor(lens, device=dev)) == want
    nbest = dec.decode_nbest(x.numpy(), lens, 3)
    for b, r in enumerate(res):
        assert [t for _, t in nbest[b]] == ["".join(EN_SP[c] for c in p) for p, _, _ in r]
        assert all(abs(s - am) <= margin_min(60) * max(1, abs(am), abs(f)) for (s, _), (_, f, am) in zip(nbest[b], r))


def _translator_fixture(tmp_path):
    """the checkpoint and audio fixture of test_gpu_ctc_beam_lm.py: a reference-style checkpoint over EN_LABELS, three tones"""
    import wave as wavmod
    from oracle import ref_cpu as R
    state = R.formula_state("plain", 29)
    for k_ in state:
        if k_.endswith("running_var"):
            state[k_] = state[k_] * 0 + 0.5 + 0.01 * torch.arange(state[k_].numel()).float() % 1.0
    ckpt = {"state_dict": {"encoder." + k_: v for k_, v in state.items()},
            "hyper_parameters": {"learning_rate": 1e-2, "weight_decay": 1e-3, "labels": EN_SP, "total_epoch": 1, "drop_rate": 0.0,
                                 "mask": True, "use_cer": False}, "epoch": 0, "global_step": 0}
    path = tmp_path / "ref_style.ckpt"
    torch.save(ckpt, path)
    wavs = []
    for i, secs in enumerate((2.0, 1.5, 2.5)):
        g = torch.Generator().manual_seed(5 + i)
        n = int(16000 * secs)
        t = torch.arange(n) / 16000.0
        y = 0.3 * torch.sin(2 * math.pi * (220 + 60 * i + 180 * t) * t) + 0.05 * torch.randn(n, generator=g)
        pcm = (y.clamp(-1, 1) * 32767).to(torch.int16)
        wp = tmp_path / ("a%d.wav" % i)
        with wavmod.open(str(wp), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000); f.writeframes(pcm.numpy().tobytes())
        wavs.append((str(wp), secs))
    return str(path), wavs


def test_translator_with_word_lm_decodes_lexicon_words_only(dev, tmp_path, en_lm):
    from lightning_asr_amd.predict import AsrTranslator
    words, path = en_lm
    ckpt, wavs = _translator_fixture(tmp_path)
    tr = AsrTranslator(ckpt, map_location="cuda", decoder="beam", beam_width=8, cutoff_top_n=40, lm_path=path, alpha=0.5, beta=1.0)
    assert tr.beam.scorer is not None and not tr.beam.scorer.is_character_based()
    wl = word_lm(path, EN_SP)
    ids = {s: i for i, s in enumerate(EN_SP)}
    for wp, _ in wavs:
        text = tr.translate(wp)
        assert wl.exists(tuple(ids[ch] for ch in text)), text          # a walk of the lexicon: whole words, then a word prefix
        assert all(w in wl.words for w in text.split(" ")[:-1])
        timed, records = tr.translate_timed(wp)
        assert wl.exists(tuple(ids[ch] for ch in timed)) and all(w in wl.words for w in timed.split(" ")[:-1])
        assert isinstance(records, list)
