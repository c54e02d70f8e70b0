"""GPU tier of the hotword-biased CTC prefix beam search (csrc/ctc_beam.hip, lasr_ctc_beam_decode_bias / _lm_bias): n-best
lists, scores and bias scores against the f64 oracle (tests/helpers/ctc_beam_bias_oracle.py), bit identity of a bank of no
phrases with the unbiased searches, the LM variant with its early cutoff, determinism, graph capture, error codes and the
Python surface (BeamSearchDecoderWithLM(hotwords=...), AsrTranslator(decoder="beam", hotwords=[...])).

As in test_gpu_ctc_beam*.py every oracle comparison first asserts that the oracle's decision margin - now including the
end-of-utterance re-ranking, and for the LM variant each early-cutoff comparison - clears margin_min(T) = 8 * 2^-24 * sqrt(T);
scores must agree to that relative tolerance.  Weights are multiples of 0.25, so every bonus is exact in f32 and bias_scores
are compared with ``==``.  Inputs are the ``peaky`` generator of those files, the first of seeds 0..31 whose margin clears."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import arpa_synth as S  # noqa: E402
import ctc_beam_bias_oracle as BO  # noqa: E402
import ctc_beam_lm_oracle as LO  # noqa: E402
import ctc_beam_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

EN = ["'"] + [chr(ord("a") + i) for i in range(26)]               # data/labels.txt: C = 28 with the blank
EN_SP = [" "] + EN                                                # predict.EN_LABELS (C = 29)
SEEDS = tuple(range(32))
E_ARG, E_WORKSPACE = -1, -3


def margin_min(T: int) -> float:
    return 8.0 * 2.0 ** -24 * math.sqrt(max(int(T), 1))


def peaky(B, T, C, seed, hot=8.0, sd=2.0, p_blank=0.6):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g) * sd
    hotc = torch.randint(0, C - 1, (B, T), generator=g)
    hotc = torch.where(torch.rand(B, T, generator=g) < p_blank, torch.full_like(hotc, C - 1), hotc)
    x.scatter_add_(2, hotc.unsqueeze(-1), torch.full((B, T, 1), float(hot)))
    return torch.log_softmax(x, -1)


def weights_for(n, w):
    return [w * (1.0, 1.5, 2.0)[i % 3] for i in range(n)]


def bank_c28(x, w, seed):
    """labels 2..5 of the unbiased second-best hypothesis of utterance 0, that phrase's first two labels (a phrase that is a
    prefix of another), the phrase extended by two labels, and 20 random phrases of 1..5 labels"""
    C = x.shape[-1]
    hyps, _ = O.beam_search(x[0].numpy(), x.shape[1], C - 1, 16, 40, 1.0, 2)
    base = list(hyps[1][0][2:6])
    assert len(base) == 4, hyps
    rng = np.random.default_rng(1000 + seed)
    phrases = [base, base[:2], base + [int(c) for c in rng.integers(0, C - 1, 2)]]
    phrases += [[int(c) for c in rng.integers(0, C - 1, int(rng.integers(1, 6)))] for _ in range(20)]
    return phrases, weights_for(len(phrases), w)


def bank_han(x, w, seed):
    """three phrases cut from the unbiased best and second-best hypotheses of utterance 0 and 40 random phrases of 1..4 labels
    drawn from the frame winners"""
    C = x.shape[-1]
    hyps, _ = O.beam_search(x[0].numpy(), x.shape[1], C - 1, 16, 40, 1.0, 2)
    best, second = list(hyps[0][0]), list(hyps[1][0])
    assert len(best) >= 4 and len(second) >= 4, hyps
    rng = np.random.default_rng(2000 + seed)
    winners = [int(c) for c in x.argmax(-1).flatten().tolist() if c != C - 1]
    phrases = [best[1:4], second[:3], second[-3:]]
    phrases += [[winners[int(i)] for i in rng.integers(0, len(winners), int(rng.integers(1, 5)))] for _ in range(40)]
    return phrases, weights_for(len(phrases), w)


_CASES = {}
COUNTS = {k: 0 for k in BO.KINDS}                                 # step kinds the oracle walked, over this file's cases


def bias_case(C, B, T, W, k, cp, n_best, w, lens=None, hot=8.0, make_bank=bank_c28, lm=None):
    """the first seed whose oracle margin clears margin_min(T), built once per argument set and left unchanged:
    (log-probs, phrases, weights, oracle n-best, early-cutoff drops)"""
    key = (C, B, T, W, k, cp, n_best, w, None if lens is None else tuple(lens), hot, make_bank.__name__, None if lm is None else lm[-1])
    if key in _CASES:
        return _CASES[key]
    worst = 0.0
    for seed in SEEDS:
        x = peaky(B, T, C, seed, hot)
        phrases, weights = make_bank(x, w, seed)
        bank = BO.Bank(phrases, weights)
        # a seed is given up at the first frame that falls short of the margin: the margin only shrinks
        res, m, fired = BO.beam_search_batch(x.numpy(), lens, C - 1, bank, W, k, cp, n_best, None if lm is None else lm[:4],
                                             stop_below=margin_min(T))
        if m >= margin_min(T):
            for kind in BO.KINDS:
                COUNTS[kind] += bank.count[kind]
            _CASES[key] = (x, phrases, weights, res, fired)
            return _CASES[key]
        worst = max(worst, m)
    raise AssertionError("no seed of 0..31 gives an oracle margin above %.2e (best %.2e)" % (margin_min(T), worst))


def run(dev, x, lens, phrases, weights, W, k, cp, n_best, lm=None):
    from lightning_asr_amd import ops
    C = x.shape[-1]
    bank = ops.build_hotwords(phrases, weights, n_classes=C, blank=C - 1, device=dev)
    lt = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    out = ops.ctc_beam_decode_biased(x.to(dev).contiguous(), lt, C - 1, bank, W, k, cp, n_best, lm)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def run_plain(dev, x, lens, W, k, cp, n_best):
    from lightning_asr_amd import ops
    lt = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    out = ops.ctc_beam_decode(x.to(dev).contiguous(), lt, x.shape[-1] - 1, W, k, cp, n_best)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def assert_matches(got, res, n_best, T):
    tok, n, sc, am, bs = got
    tol = margin_min(T)
    for b, hyps in enumerate(res):
        for j in range(n_best):
            if j < len(hyps):
                want, score, am_want, fb = hyps[j]
                assert n[b, j] == len(want), (b, j, n[b, j], len(want))
                assert tuple(int(c) for c in tok[b, j, :n[b, j]]) == want, (b, j)
                assert (tok[b, j, n[b, j]:] == -1).all()
                assert bs[b, j] == fb, (b, j, float(bs[b, j]), fb)
                assert abs(sc[b, j] - score) <= tol * max(1.0, abs(score)), (b, j, float(sc[b, j]), score)
                assert abs(am[b, j] - am_want) <= tol * max(1.0, abs(am_want), abs(score)), (b, j, float(am[b, j]), am_want)
            else:
                assert n[b, j] == -1 and sc[b, j] == -np.inf and am[b, j] == -np.inf and bs[b, j] == 0 and (tok[b, j] == -1).all()


def tokens_differ(a_tok, a_n, b_tok, b_n):
    return not (np.array_equal(a_n, b_n) and np.array_equal(a_tok, b_tok))


# Candidates per thread (cutoff_top_n above C acts as C = 28): 1 at W 1, 2 at W 16, 8 at W 64 and at (W 128, k 8), 16 at
# (W 128, k 40); test_bias_large_vocabulary adds 4 and 33, so the file runs every rung of the ladder.
C28_SHAPES = [(1, 40, 1.0), (16, 40, 1.0), (64, 40, 0.95), (128, 8, 1.0), (128, 40, 1.0)]
C28_CASES = [(W, k, cp, w) for W, k, cp in C28_SHAPES for w in (1.0, 2.0, 4.0, 8.0)]


@pytest.mark.parametrize("W,k,cp,w", C28_CASES)
def test_bias_matches_oracle_c28(dev, W, k, cp, w):
    B, T, C = 2, 50, 28
    n_best = min(W, 4)
    x, phrases, weights, res, _ = bias_case(C, B, T, W, k, cp, n_best, w)
    got = run(dev, x, None, phrases, weights, W, k, cp, n_best)
    plain = run_plain(dev, x, None, W, k, cp, n_best)
    assert tokens_differ(got[0], got[1], plain[0], plain[1])          # the bank changes the result
    assert_matches(got, res, n_best, T)


@pytest.mark.parametrize("W", [16, 128])
def test_bias_large_vocabulary(dev, W):
    """C = 4334: the radix-select pruning, the J = 33 kernel at W = 128, phrases over label ids up to 4332"""
    B, T, C = 2, 30, 4334
    x, phrases, weights, res, _ = bias_case(C, B, T, W, 40, 1.0, 4, 2.0, hot=12.0, make_bank=bank_han)
    got = run(dev, x, None, phrases, weights, W, 40, 1.0, 4)
    plain = run_plain(dev, x, None, W, 40, 1.0, 4)
    assert tokens_differ(got[0], got[1], plain[0], plain[1])
    assert_matches(got, res, 4, T)


def test_bias_ragged_lengths(dev):
    B, T, W = 6, 40, 16
    lens = [40, 0, 1, 17, 33, 2]
    x, phrases, weights, res, _ = bias_case(28, B, T, W, 40, 1.0, 3, 2.0, lens=lens)
    got = run(dev, x, lens, phrases, weights, W, 40, 1.0, 3)
    assert_matches(got, res, 3, T)
    assert got[1][1, 0] == 0 and got[2][1, 0] == 0.0 and got[4][1, 0] == 0.0       # lens 0: the empty hypothesis, score 0, no bias


def test_every_step_kind_was_exercised(dev):
    """over the cases above (built here when this test runs alone) the oracle took every kind of step"""
    for W, k, cp, w in C28_CASES:
        bias_case(28, 2, 50, W, k, cp, min(W, 4), w)
    for W in (16, 128):
        bias_case(4334, 2, 30, W, 40, 1.0, 4, 2.0, hot=12.0, make_bank=bank_han)
    bias_case(28, 6, 40, 16, 40, 1.0, 3, 2.0, lens=[40, 0, 1, 17, 33, 2])
    assert all(v > 0 for v in COUNTS.values()), COUNTS


# ------------------------------------------------------------------------------------------------ a bank of no phrases
@pytest.mark.parametrize("C,W,k,cp", [(28, 1, 40, 1.0), (28, 16, 40, 0.95), (28, 64, 40, 1.0), (28, 128, 8, 1.0), (28, 128, 40, 1.0),
                                      (4334, 16, 40, 1.0), (4334, 128, 40, 1.0)])
def test_empty_bank_is_the_unbiased_search_bit_for_bit(dev, C, W, k, cp):
    B, T = 4, 60
    lens = [60, 33, 0, 59]
    x = peaky(B, T, C, 11, 8.0 if C == 28 else 12.0)
    n_best = min(W, 8)
    got = run(dev, x, lens, [], [], W, k, cp, n_best)
    plain = run_plain(dev, x, lens, W, k, cp, n_best)
    for u, v in zip(got[:3], plain):
        assert np.array_equal(u, v)
    assert np.array_equal(got[3], plain[2]) and (got[4] == 0).all()


@pytest.fixture(scope="module")
def en_lms(tmp_path_factory):
    d = tmp_path_factory.mktemp("en_lm_bias")
    return {o: S.write_arpa(d / ("en%d.arpa" % o), EN, o, 400, seed=o) for o in (2, 3, 6)}


@pytest.mark.parametrize("order,W,k", [(2, 16, 40), (3, 128, 40), (6, 64, 8)])
def test_empty_bank_is_the_lm_search_bit_for_bit(dev, en_lms, order, W, k):
    from lightning_asr_amd import ops
    B, T, C = 4, 60, 28
    lens = torch.tensor([60, 33, 0, 59], dtype=torch.int32, device=dev)
    x = peaky(B, T, C, 12).to(dev).contiguous()
    lm = ops.load_arpa(en_lms[order], EN, dev, 0.7, 1.5)            # beta 1.5: the early cutoff is at work
    bank = ops.build_hotwords([], n_classes=C, blank=C - 1, device=dev)
    got = ops.ctc_beam_decode_biased(x, lens, C - 1, bank, W, k, 1.0, 8, lm)
    want = ops.ctc_beam_decode_lm(x, lens, C - 1, lm, W, k, 1.0, 8)
    torch.cuda.synchronize()
    for u, v in zip(got[:4], want):
        assert torch.equal(u, v)
    assert (got[4] == 0).all()


# ------------------------------------------------------------------------------------------------ LM + bias
def lm_run(dev, case, path, W, k, n_best, alpha, beta):
    from lightning_asr_amd import ops
    x, phrases, weights, res, fired = case
    lm = ops.load_arpa(path, EN, dev, alpha, beta)
    return run(dev, x, None, phrases, weights, W, k, 1.0, n_best, lm)


@pytest.mark.parametrize("order,W,alpha,beta", [(2, 16, 1.0, 1.0), (3, 16, 0.5, -0.5), (6, 16, 0.8, 1.5), (2, 128, 0.5, 0.5),
                                                (3, 128, 1.0, 2.0), (6, 128, 0.3, -1.0)])
def test_lm_bias_matches_oracle(dev, en_lms, order, W, alpha, beta):
    B, T, C = 2, 50, 28
    path = en_lms[order]
    lm = (EN, LO.ArpaOracle.from_file(path), alpha, beta, (path, alpha, beta))
    case = bias_case(C, B, T, W, 40, 1.0, 4, 2.0, lm=lm)
    assert_matches(lm_run(dev, case, path, W, 40, 4, alpha, beta), case[3], 4, T)


def test_lm_bias_early_cutoff_decides(dev, en_lms):
    """beta = 4 on a full beam and a light bank (w 0.25: max_credit 3): comparisons fire even with the max_credit slack in the
    cutoff, and the oracle without the early cutoff returns other scores (or hypotheses); the kernel matches the oracle with it"""
    B, T, C, W, alpha, beta = 2, 50, 28, 16, 0.5, 4.0
    path = en_lms[3]
    arpa = LO.ArpaOracle.from_file(path)
    case = bias_case(C, B, T, W, 40, 1.0, 4, 0.25, lm=(EN, arpa, alpha, beta, (path, alpha, beta)))
    x, phrases, weights, res, fired = case
    assert fired > 0
    res_nf, _, _ = BO.beam_search_batch(x.numpy(), None, C - 1, BO.Bank(phrases, weights), W, 40, 1.0, 4, (EN, arpa, alpha, beta),
                                        use_filter=False)
    differs = any(a[0] != b[0] or abs(a[1] - b[1]) > 100 * margin_min(T) * max(1.0, abs(a[1]))
                  for ra, rb in zip(res, res_nf) for a, b in zip(ra, rb))
    assert differs
    assert_matches(lm_run(dev, case, path, W, 40, 4, alpha, beta), res, 4, T)


SYM47 = EN + [chr(ord("A") + i) for i in range(20)]               # 47 labels: C = 48, the smallest with 41 classes to keep


# The LM + hotword search at the rungs test_lm_bias_matches_oracle (J = 2 and 16) leaves out: W 8, 32 and 64 on C = 28 are 1, 4
# and 8 candidates per thread; C = 48 keeps cutoff_top_n = 40 labels, and W = 128 then has 128 * 41 candidates: J = 33.
@pytest.mark.parametrize("vocab,order,W,alpha,beta", [(EN, 2, 8, 1.0, 1.0), (EN, 3, 32, 0.5, -0.5), (EN, 6, 64, 0.8, 1.5),
                                                      (SYM47, 3, 128, 0.5, 0.5)], ids=["J1", "J4", "J8", "J33"])
def test_lm_bias_every_other_rung(dev, en_lms, tmp_path, vocab, order, W, alpha, beta):
    from lightning_asr_amd import ops
    B, T, C = 2, 30, len(vocab) + 1
    path = en_lms[order] if vocab is EN else S.write_arpa(tmp_path / "sym47.arpa", vocab, order, 400, seed=order)
    lm = (vocab, LO.ArpaOracle.from_file(path), alpha, beta, (path, alpha, beta))
    x, phrases, weights, res, _ = bias_case(C, B, T, W, 40, 1.0, 4, 2.0, lm=lm)
    got = run(dev, x, None, phrases, weights, W, 40, 1.0, 4, ops.load_arpa(path, vocab, dev, alpha, beta))
    assert_matches(got, res, 4, T)


# ------------------------------------------------------------------------------------------------ determinism, capture, errors
@pytest.mark.parametrize("with_lm", [False, True])
def test_bias_deterministic_and_graph_capture(dev, en_lms, with_lm):
    from lightning_asr_amd import ops
    B, T, C = 8, 120, 28
    x = peaky(B, T, C, 5).to(dev).contiguous()
    lens = torch.tensor([120, 90, 1, 0, 119, 77, 100, 120], dtype=torch.int32, device=dev)
    phrases, weights = bank_c28(x.cpu(), 2.0, 5)
    bank = ops.build_hotwords(phrases, weights, n_classes=C, blank=C - 1, device=dev)
    lm = ops.load_arpa(en_lms[6], EN, dev, 0.8, 1.0) if with_lm else None
    a = ops.ctc_beam_decode_biased(x, lens, C - 1, bank, 32, 40, 0.95, 8, lm)
    b = ops.ctc_beam_decode_biased(x, lens, C - 1, bank, 32, 40, 0.95, 8, lm)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.ctc_beam_decode_biased(x, lens, C - 1, bank, 32, 40, 0.95, 8, lm)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = ops.ctc_beam_decode_biased(x, lens, C - 1, bank, 32, 40, 0.95, 8, lm)
    g.replay()
    torch.cuda.synchronize()
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    assert (a[4] > 0).any()                                          # the bank is applied


def test_wrong_image_and_bad_arguments(dev, en_lms):
    from lightning_asr_amd import _lib, ops
    lib = _lib.load()
    B, T, C, W, nb = 2, 10, 28, 4, 2
    x = peaky(B, T, C, 0).to(dev).contiguous()
    lm = ops.load_arpa(en_lms[2], EN, dev, 1.0, 1.0)
    bank = ops.build_hotwords([[1, 2]], n_classes=C, blank=C - 1, device=dev)
    other = ops.build_hotwords([[1, 2]], n_classes=C + 1, blank=C, device=dev)     # a bank for another vocabulary
    nbytes = int(lib.lasr_ctc_beam_workspace_bytes(B, T, C, W, 28))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                     # noqa: E731

    def fresh():
        return (torch.full((B, nb, T), 7, dtype=torch.int32, device=dev), torch.full((B, nb), 7, dtype=torch.int32, device=dev),
                torch.full((B, nb), 7.0, device=dev), torch.full((B, nb), 7.0, device=dev), torch.full((B, nb), 7.0, device=dev))

    def call(img, lm_img=None, **kw):
        a = dict(blank=C - 1, W=W, cp=1.0, n_best=nb, ws_bytes=nbytes, bias_out=True)
        a.update(kw)
        tok, n, sc, am, bs = out = fresh()
        head = (P(x), None, B, T, C, a["blank"], a["W"], 28, a["cp"], a["n_best"])
        tail = (P(tok), P(n), P(sc), P(am), P(bs) if a["bias_out"] else None, P(ws), a["ws_bytes"], None)
        if lm_img is None:
            rc = lib.lasr_ctc_beam_decode_bias(*head, img, *tail)
        else:
            rc = lib.lasr_ctc_beam_decode_lm_bias(*head, lm_img, a.get("alpha", 1.0), 1.0, img, *tail)
        torch.cuda.synchronize()
        return rc, out

    def untouched(out):
        return all(bool((t == 7).all()) for t in out)

    def empty(out):
        tok, n, sc, am, bs = out
        return bool((tok == -1).all() and (n == -1).all() and (sc == -math.inf).all() and (am == -math.inf).all() and (bs == 0).all())

    rc, out = call(P(bank.image))
    assert rc == 0 and not empty(out) and not untouched(out)
    # images that are no hotword image for these classes: empty slots
    for img in (lm.image, other.image, torch.zeros(256, dtype=torch.uint8, device=dev)):
        rc, out = call(P(img))
        assert rc == 0 and empty(out)
    rc, out = call(P(bank.image), P(lm.image))
    assert rc == 0 and not empty(out)
    rc, out = call(P(lm.image), P(lm.image))                         # a wrong bias image
    assert rc == 0 and empty(out)
    rc, out = call(P(bank.image), P(bank.image))                     # a wrong LM image
    assert rc == 0 and empty(out)
    # bad arguments: LASR_E_ARG (LASR_E_WORKSPACE for a short workspace), nothing launched
    for kw in (dict(blank=C), dict(n_best=W + 1), dict(n_best=0), dict(cp=0.0), dict(cp=1.5), dict(bias_out=False)):
        for lm_img in (None, P(lm.image)):
            rc, out = call(P(bank.image), lm_img, **kw)
            assert rc == E_ARG and untouched(out), kw
    rc, out = call(None)
    assert rc == E_ARG and untouched(out)
    rc, out = call(None, P(lm.image))
    assert rc == E_ARG and untouched(out)
    rc, out = call(P(bank.image), P(lm.image), alpha=math.nan)
    assert rc == E_ARG and untouched(out)
    rc, out = call(P(bank.image), ws_bytes=nbytes - 1)
    assert rc == E_WORKSPACE and untouched(out)
    # the Python checks in front of them
    with pytest.raises(ValueError, match="built for 29 classes"):
        ops.ctc_beam_decode_biased(x, None, C - 1, other, W)
    with pytest.raises(ValueError, match="image is on"):
        ops.ctc_beam_decode_biased(x, None, C - 1, ops.build_hotwords([[1]], n_classes=C, blank=C - 1, device="cpu"), W)
    with pytest.raises(TypeError):
        ops.ctc_beam_decode_biased(x, None, C - 1, lm, W)


# ------------------------------------------------------------------------------------------------ Python surface
def test_decoder_with_hotwords(dev, en_lms):
    from lightning_asr_amd import ops
    from lightning_asr_amd.beam_search import BeamSearchDecoderWithLM, parse_hotwords
    B, T, W = 3, 60, 16
    lens = [60, 45, 12]
    x = peaky(B, T, 28, 3)
    hyps, _ = O.beam_search(x[0].numpy(), T, 27, 16, 40, 1.0, 2)
    second = "".join(EN[c] for c in hyps[1][0])
    hot = [second[2:6], (second[:3], 1.5), "zq"]
    dec = BeamSearchDecoderWithLM(EN, W, 1.0, 1.0, None, 4, cutoff_prob=1.0, cutoff_top_n=40, hotwords=hot, hotword_weight=4.0)
    assert dec.hotwords.n_phrases == 3 and "starting value" in BeamSearchDecoderWithLM.__init__.__doc__
    phrases, weights = parse_hotwords(EN, hot, 4.0)
    assert weights == [4.0, 1.5, 4.0]
    bank = ops.build_hotwords(phrases, weights, n_classes=28, blank=27, device=dev)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    want = ops.ctc_beam_decode_biased(x.to(dev), lt, 27, bank, W, 40, 1.0, 3)
    got = dec.search_full(x.numpy(), np.array(lens), 3)
    assert len(got) == 4
    for u, v in zip(got, want[:4]):
        assert torch.equal(u, v)                                     # the fourth element: the acoustic scores
    plain = ops.ctc_beam_decode(x.to(dev), lt, 27, W, 40, 1.0, 3)
    assert not torch.equal(plain[0], got[0])
    texts = dec.forward(x.numpy(), np.array(lens))
    tok, n = want[0].cpu().numpy(), want[1].cpu().numpy()
    assert texts == ["".join(EN[c] for c in tok[b, 0, :n[b, 0]]) for b in range(B)]
    nbest = dec.decode_nbest(x.numpy(), lens, 3)
    assert [s for s, _ in nbest[0]] == [float(v) for v in want[3][0].cpu()]
    # [] and None switch the biasing off: the unbiased calls and results, exactly
    for off in ([], None):
        dec.set_hotwords(off)
        assert dec.hotwords is None
        back = dec.search_full(x.numpy(), np.array(lens), 3)
        assert back[3] is None and all(torch.equal(u, v) for u, v in zip(back[:3], plain))
        dec.set_hotwords(hot, 4.0)
        assert torch.equal(dec.search(x.numpy(), np.array(lens), 3)[0], want[0])
    with pytest.raises(ValueError, match="'é'"):
        dec.set_hotwords(["café"])
    assert dec.hotwords is not None                                  # a rejected list leaves the bank in place
    # with a character LM the bank is swapped without reloading it
    dlm = BeamSearchDecoderWithLM(EN, W, 0.7, 1.0, en_lms[3], 4, hotwords=hot)
    scorer = dlm.scorer
    a = dlm.search_full(x.numpy(), np.array(lens), 3)
    want_lm = ops.ctc_beam_decode_biased(x.to(dev), lt, 27, dlm.hotwords, W, 40, 1.0, 3, scorer, 0.7, 1.0)
    assert all(torch.equal(u, v) for u, v in zip(a, want_lm[:4]))
    dlm.set_hotwords(None)
    assert dlm.scorer is scorer
    b = dlm.search_full(x.numpy(), np.array(lens), 3)
    assert all(torch.equal(u, v) for u, v in zip(b, ops.ctc_beam_decode_lm(x.to(dev), lt, 27, scorer, W, 40, 1.0, 3, 0.7, 1.0)))


def _translator_fixture(tmp_path):
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
    g = torch.Generator().manual_seed(5)
    n = 32000
    t = torch.arange(n) / 16000.0
    y = 0.3 * torch.sin(2 * math.pi * (220 + 180 * t) * t) + 0.05 * torch.randn(n, generator=g)
    y[14000:20000] *= 0.001                                          # a pause: translate_long cuts two segments
    pcm = (y.clamp(-1, 1) * 32767).to(torch.int16)
    wp = tmp_path / "a.wav"
    with wavmod.open(str(wp), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000); f.writeframes(pcm.numpy().tobytes())
    return str(path), str(wp)


def test_translator_with_hotwords(dev, tmp_path, en_lms):
    from lightning_asr_amd import ops
    from lightning_asr_amd.predict import AsrTranslator
    ckpt, wp = _translator_fixture(tmp_path)
    with pytest.raises(ValueError, match="beam"):
        AsrTranslator(ckpt, map_location="cuda", decoder="greedy", hotwords=["ab"])
    tr = AsrTranslator(ckpt, map_location="cuda", decoder="beam", beam_width=8, hotwords=["ab", ("it's a", 3.0)], hotword_weight=2.5)
    assert tr.beam.hotwords.n_phrases == 2
    # record what the translator hands to the search and what comes back
    seen = []
    inner = tr.beam.search_full

    def recording(log_probs, lens, n_best=1):
        out = inner(log_probs, lens, n_best)
        seen.append((log_probs.detach().float().clone(), None if lens is None else lens.clone(), n_best, out))
        return out
    tr.beam.search_full = recording

    def check():
        """every recorded call is the ops call on the same log-probs with the translator's bank; returns the texts"""
        texts = []
        for lp, lens, n_best, out in seen:
            want = ops.ctc_beam_decode_biased(lp.contiguous(), None if lens is None else lens.to(torch.int32), lp.shape[-1] - 1,
                                              tr.beam.hotwords, 8, 40, 1.0, n_best)
            assert all(torch.equal(u, v) for u, v in zip(out, want[:4]))
            tok, n = want[0].cpu().numpy(), want[1].cpu().numpy()
            texts += [["".join(EN_SP[c] for c in tok[b, j, :max(n[b, j], 0)]) for j in range(n_best) if n[b, j] >= 0]
                      for b in range(tok.shape[0])]
        return texts
    text = tr.translate(wp)
    assert len(seen) == 1 and check() == [[text]]
    seen.clear()
    nb = tr.translate_nbest(wp, 3)
    assert len(seen) == 1 and check() == [[t for t, _ in nb]]
    seen.clear()
    res = tr.translate_long(wp, timed=False)
    assert len(seen) >= 1 and sorted(t[0] for t in check()) == sorted(s["text"] for s in res["segments"])
    # the hotwords of the best hypothesis, weighted up: its bias score is positive
    tr.beam.search_full = inner
    seen.clear()
    if len(text) >= 2:
        tr.set_hotwords([text[:min(len(text), 4)]], 1.0)
        lp = tr.model._encode(tr.audio_parser.parse_audio(wp, mask=False), torch.ones(1, device=dev)).float()
        out = ops.ctc_beam_decode_biased(lp.contiguous(), None, 28, tr.beam.hotwords, 8, 40, 1.0, 1)
        assert float(out[4][0, 0]) > 0
    tr.set_hotwords(None)
    assert tr.beam.hotwords is None and isinstance(tr.translate(wp), str)
    # a word-level LM and hotwords: not implemented
    wpath = tmp_path / "words.arpa"
    wpath.write_text("\\data\\\nngram 1=4\n\n\\1-grams:\n-1.0\t<s>\n-1.0\t</s>\n-0.5\tab\n-0.6\tba\n\n\\end\\\n")
    with pytest.raises(NotImplementedError):
        AsrTranslator(ckpt, map_location="cuda", decoder="beam", lm_path=str(wpath), hotwords=["ab"])
    wtr = AsrTranslator(ckpt, map_location="cuda", decoder="beam", lm_path=str(wpath))
    with pytest.raises(NotImplementedError):
        wtr.set_hotwords(["ab"])
    with pytest.raises(NotImplementedError):
        ops.ctc_beam_decode_biased(torch.zeros(1, 4, 29, device=dev), None, 28, ops.build_hotwords([[1]], n_classes=29, blank=28, device=dev),
                                   4, lm=wtr.beam.scorer)
