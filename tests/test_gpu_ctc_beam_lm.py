"""GPU tier of the LM-fused CTC prefix beam search (csrc/ctc_beam.hip, lasr_ctc_beam_decode_lm): n-best lists against the f64
oracle (tests/helpers/ctc_beam_lm_oracle.py) over synthetic character ARPA LMs (tests/helpers/arpa_synth.py), a case where the
early cutoff decides the result, determinism, graph capture, and the Python surface (BeamSearchDecoderWithLM(lm_path=...),
AsrTranslator(decoder="beam", lm_path=...)).

As in test_gpu_ctc_beam.py, every oracle comparison first asserts that the oracle's decision margin (now including each
early-cutoff comparison) clears margin_min(T); scores must agree to that relative tolerance."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import arpa_synth as S  # noqa: E402
import ctc_beam_lm_oracle as LO  # noqa: E402

pytestmark = pytest.mark.gpu

EN = ["'"] + [chr(ord("a") + i) for i in range(26)]               # data/labels.txt: C = 28 with the blank
EN_SP = [" "] + EN                                                # predict.EN_LABELS (C = 29): " " is never an ARPA word (OOV)
HAN = [chr(0x4E00 + i) for i in range(4333)]                      # an AISHELL-sized vocabulary, C = 4334


def margin_min(T: int) -> float:
    return 8.0 * 2.0 ** -24 * math.sqrt(max(int(T), 1))


def peaky(B, T, C, seed, hot=8.0, sd=2.0, p_blank=0.6):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g) * sd
    hotc = torch.randint(0, C - 1, (B, T), generator=g)
    hotc = torch.where(torch.rand(B, T, generator=g) < p_blank, torch.full_like(hotc, C - 1), hotc)
    x.scatter_add_(2, hotc.unsqueeze(-1), torch.full((B, T, 1), float(hot)))
    return torch.log_softmax(x, -1)


def lm_case(vocab, path, B, T, W, k, cp, n_best, alpha, beta, lens=None, hot=8.0, seeds=tuple(range(32))):
    """the first seed whose oracle margin clears margin_min(T): (log-probs, oracle n-best, early-cutoff drops)"""
    lm = LO.ArpaOracle.from_file(path)
    C = len(vocab) + 1
    worst = 0.0
    for seed in seeds:
        x = peaky(B, T, C, seed, hot)
        res, m, fired = LO.beam_search_batch(x.numpy(), lens, C - 1, vocab, lm, alpha, beta, W, k, cp, n_best)
        if m >= margin_min(T):
            return x, res, fired
        worst = max(worst, m)
    raise AssertionError("no seed of %s gives an oracle margin above %.2e (best %.2e)" % (seeds, margin_min(T), worst))


def run(dev, x, lens, vocab, path, W, k, cp, n_best, alpha, beta):
    from lightning_asr_amd import ops
    lm = ops.load_arpa(path, vocab, dev, alpha, beta)
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
                want, fused, approx = hyps[j]
                assert n[b, j] == len(want), (b, j, n[b, j], len(want))
                assert tuple(int(c) for c in tok[b, j, :n[b, j]]) == want, (b, j)
                assert (tok[b, j, n[b, j]:] == -1).all()
                assert abs(sc[b, j] - fused) <= tol * max(1.0, abs(fused)), (b, j, float(sc[b, j]), fused)
                assert abs(am[b, j] - approx) <= tol * max(1.0, abs(approx), abs(fused)), (b, j, float(am[b, j]), approx)
            else:
                assert n[b, j] == -1 and sc[b, j] == -np.inf and am[b, j] == -np.inf and (tok[b, j] == -1).all(), (b, j)


@pytest.fixture(scope="module")
def en_lms(tmp_path_factory):
    d = tmp_path_factory.mktemp("en_lm")
    return {o: S.write_arpa(d / ("en%d.arpa" % o), EN, o, 400, seed=o) for o in (1, 2, 3, 6)}


# (order, W, k, cutoff_prob, alpha, beta): every order, width and sign of beta, cutoff_prob < 1
EN_CASES = [(1, 16, 40, 1.0, 0.5, 0.0), (2, 1, 40, 1.0, 1.0, 1.0), (2, 64, 40, 1.0, 0.5, -0.5), (3, 16, 40, 1.0, 1.0, 2.0),
            (3, 64, 40, 0.95, 0.8, 1.0), (3, 128, 8, 1.0, 0.5, 0.5), (6, 16, 40, 1.0, 1.0, 1.5), (6, 128, 40, 1.0, 0.3, -1.0),
            (1, 64, 40, 0.95, 1.0, 2.5), (6, 1, 8, 0.95, 2.0, 0.0)]


@pytest.mark.parametrize("order,W,k,cp,alpha,beta", EN_CASES)
def test_beam_lm_matches_oracle_c28(dev, en_lms, order, W, k, cp, alpha, beta):
    B, T = 2, 50
    n_best = min(W, 4)
    x, res, _ = lm_case(EN, en_lms[order], B, T, W, k, cp, n_best, alpha, beta)
    assert_matches(run(dev, x, None, EN, en_lms[order], W, k, cp, n_best, alpha, beta), res, n_best, T)


def test_beam_lm_early_cutoff_decides(dev, en_lms):
    """beta = 2.5 on a full beam: the oracle without the early cutoff returns other scores (or hypotheses); the kernel matches
    the oracle with it"""
    B, T, W, alpha, beta = 2, 50, 16, 0.5, 2.5
    path = en_lms[3]
    x, res, fired = lm_case(EN, path, B, T, W, 40, 1.0, 4, alpha, beta)
    assert fired > 0
    lm = LO.ArpaOracle.from_file(path)
    res_nf, _, _ = LO.beam_search_batch(x.numpy(), None, len(EN), EN, lm, alpha, beta, W, 40, 1.0, 4, use_filter=False)
    differs = any(a[0] != b[0] or abs(a[1] - b[1]) > 100 * margin_min(T) * max(1.0, abs(a[1]))
                  for ra, rb in zip(res, res_nf) for a, b in zip(ra, rb))
    assert differs
    assert_matches(run(dev, x, None, EN, path, W, 40, 1.0, 4, alpha, beta), res, 4, T)


def test_beam_lm_ragged_lengths(dev, en_lms):
    B, T, W = 6, 40, 16
    lens = [40, 0, 1, 17, 33, 2]
    x, res, _ = lm_case(EN, en_lms[3], B, T, W, 40, 1.0, 3, 1.0, 1.0, lens=lens)
    got = run(dev, x, lens, EN, en_lms[3], W, 40, 1.0, 3, 1.0, 1.0)
    assert_matches(got, res, 3, T)
    assert got[1][1, 0] == 0 and got[2][1, 0] == 0.0                  # lens 0: the empty hypothesis, fused score 0


def test_beam_lm_large_vocabulary_with_oov(dev, tmp_path):
    """C = 4334: the LM covers 3000 of the labels, the rest are OOV"""
    path = S.write_arpa(tmp_path / "han.arpa", HAN, 3, 3000, seed=5, missing=HAN[3000:])
    B, T, W = 2, 120, 16
    x, res, _ = lm_case(HAN, path, B, T, W, 40, 1.0, 4, 0.7, 1.0, hot=16.0, seeds=(0, 1, 2, 3))
    assert (x.argmax(-1) >= 3000).logical_and(x.argmax(-1) < 4333).any()   # OOV labels are among the frames' hot classes
    assert_matches(run(dev, x, None, HAN, path, W, 40, 1.0, 4, 0.7, 1.0), res, 4, T)


def test_beam_lm_widest_candidate_set(dev, tmp_path):
    """C = 4334, beam 128, cutoff_top_n 40: W * (K + 1) > 4096 candidates per frame selects the J = 33 kernel, the only one
    whose last probe group is partial"""
    path = S.write_arpa(tmp_path / "han.arpa", HAN, 3, 3000, seed=5, missing=HAN[3000:])
    B, T, W, k = 2, 40, 128, 40
    assert W * (k + 1) > 16 * 256
    x, res, fired = lm_case(HAN, path, B, T, W, k, 1.0, 8, 0.7, 1.0, hot=12.0, seeds=tuple(range(8)))
    assert fired > 0
    assert_matches(run(dev, x, None, HAN, path, W, k, 1.0, 8, 0.7, 1.0), res, 8, T)


def test_beam_lm_long_batch(dev, tmp_path):
    """one T' = 801 batch of 32 (an LM that covers every label).  Over 32 x 801 frames a few utterances always hold some
    decision closer than f32 can settle, so each utterance is held to the oracle where its own margin clears margin_min(T),
    and at least half of them must (23 of 32 do)"""
    B, T, W = 32, 801, 4
    vocab = EN
    path = S.write_arpa(tmp_path / "en3_full.arpa", vocab, 3, 400, seed=3)
    lm = LO.ArpaOracle.from_file(path)
    lens = [T] + [int(v) for v in np.random.default_rng(2).integers(600, T + 1, B - 1)]
    x = peaky(B, T, len(vocab) + 1, 0, 16.0)
    got = run(dev, x, lens, vocab, path, W, 8, 1.0, 2, 0.5, 1.0)
    ok = 0
    for b in range(B):
        hyps, m, _ = LO.beam_search(x[b].numpy(), lens[b], len(vocab), vocab, lm, 0.5, 1.0, W, 8, 1.0, 2)
        if m >= margin_min(T):
            ok += 1
            assert_matches([g[b:b + 1] for g in got], [hyps], 2, T)
    assert ok >= B // 2, ok


def test_beam_lm_deterministic_and_graph_capture(dev, en_lms):
    from lightning_asr_amd import ops
    B, T, C = 8, 200, 28
    x = peaky(B, T, C, 5).to(dev).contiguous()
    lens = torch.tensor([200, 150, 1, 0, 199, 77, 120, 200], dtype=torch.int32, device=dev)
    lm = ops.load_arpa(en_lms[6], EN, dev, 0.8, 1.0)
    a = ops.ctc_beam_decode_lm(x, lens, C - 1, lm, 32, 40, 0.95, 8)
    b = ops.ctc_beam_decode_lm(x, lens, C - 1, lm, 32, 40, 0.95, 8)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.ctc_beam_decode_lm(x, lens, C - 1, lm, 32, 40, 0.95, 8)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = ops.ctc_beam_decode_lm(x, lens, C - 1, lm, 32, 40, 0.95, 8)
    g.replay()
    torch.cuda.synchronize()
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    # the LM-free search is a different result on the same inputs (the LM is applied)
    t0, _, _ = ops.ctc_beam_decode(x, lens, C - 1, 32, 40, 0.95, 8)
    assert not torch.equal(t0, a[0])


# ------------------------------------------------------------------------------------------------ Python surface
def test_decoder_with_lm_path(dev, en_lms):
    from lightning_asr_amd.beam_search import BeamSearchDecoderWithLM
    path = en_lms[3]
    x, res, _ = lm_case(EN, path, 3, 60, 16, 40, 1.0, 3, 1.0, 1.0, lens=[60, 45, 12])
    dec = BeamSearchDecoderWithLM(EN, 16, 1.0, 1.0, path, 4, cutoff_prob=1.0, cutoff_top_n=40)
    assert dec.scorer.order == 3 and dec.scorer.is_character_based()
    want = ["".join(EN[c] for c in r[0][0]) for r in res]
    assert dec.forward(x.numpy(), np.array([60, 45, 12])) == want
    assert dec(x.to(dev), torch.tensor([60, 45, 12], device=dev)) == want
    nbest = dec.decode_nbest(x.numpy(), [60, 45, 12], 3)
    for b, r in enumerate(res):
        assert [t for _, t in nbest[b]] == ["".join(EN[c] for c in p) for p, _, _ in r]
        assert all(abs(s - am) <= margin_min(60) * max(1, abs(am), abs(f)) for (s, _), (_, f, am) in zip(nbest[b], r))


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
    man = tmp_path / "m.json"
    with open(man, "w") as f:
        for (wp, secs), text in zip(wavs, ("a b", "hello", "it's a test")):
            f.write(json.dumps({"audio_filepath": wp, "duration": secs, "text": text}) + "\n")
    return str(path), wavs, str(man)


def test_translator_beam_lm_matches_oracle(dev, tmp_path, en_lms):
    from lightning_asr_amd.predict import AsrTranslator
    from lightning_asr_amd.utils.asr_metrics import word_error_rate
    ckpt, wavs, man = _translator_fixture(tmp_path)
    W, path = 4, en_lms[2]
    tr = AsrTranslator(ckpt, map_location="cuda", decoder="beam", beam_width=W, cutoff_top_n=40, lm_path=path, alpha=0.5, beta=1.0)
    assert tr.beam.scorer is not None
    wp = wavs[0][0]
    dith = tr.audio_parser.device_dither()
    step0 = dith.step.clone()
    inputs = tr.audio_parser.parse_audio(wp, mask=False)
    with torch.no_grad():
        lp = tr.model._encode(inputs, torch.ones(1, device=dev)).float().cpu().numpy()
    lm = LO.ArpaOracle.from_file(path)
    # the first (beam, weights) whose oracle margin clears: the log-probs of this fixture are fixed, so this is a fixed choice
    tried = []
    for W in (4, 8, 16, 3, 32):
        for alpha, beta in [(0.5, 1.0), (0.3, 0.5), (1.0, 0.0), (0.8, -0.5), (0.2, 2.0)]:
            res, m, _ = LO.beam_search_batch(lp, None, len(EN_SP), EN_SP, lm, alpha, beta, W, 40, 1.0, 3)
            tried.append(m)
            if m >= margin_min(lp.shape[1]):
                break
        if m >= margin_min(lp.shape[1]):
            break
    assert m >= margin_min(lp.shape[1]), tried
    tr.beam.alpha, tr.beam.beta, tr.beam.beam_width = alpha, beta, W
    dith.step.copy_(step0)                       # the same dither draw again: the same features and log-probs
    text = tr.translate(wp)
    assert text == "".join(EN_SP[c] for c in res[0][0][0])
    dith.step.copy_(step0)
    nb = tr.translate_nbest(wp, 3)
    assert [t for t, _ in nb] == ["".join(EN_SP[c] for c in p) for p, _, _ in res[0]]

    # evalute_manifest(decoder="beam") with the LM: record the log-probs it hands to the search, hold its predictions to the
    # oracle on exactly those
    seen = []
    search = tr.beam.search

    def recording(log_probs, lens, n_best=1):
        seen.append((log_probs.float().cpu().numpy(), lens.cpu().numpy()))
        return search(log_probs, lens, n_best)
    tr.beam.search = recording
    tr.evalute_manifest(man, batch_size=2)
    utts = [(lp_b[i], int(ln[i])) for lp_b, ln in seen for i in range(lp_b.shape[0])]
    assert len(utts) == 3

    def clearing(W_, a_, b_):
        return [LO.beam_search(u, n_, len(EN_SP), EN_SP, lm, a_, b_, W_, 40, 1.0, 1)[1] >= margin_min(n_) for u, n_ in utts]
    # the first (beam, weights) under which most utterances clear the margin (the fixture's log-probs are fixed)
    grid = [(W_, a_, b_) for W_ in (4, 8, 16, 3) for a_, b_ in [(0.5, 1.0), (0.3, 0.5), (1.0, 0.0), (0.8, -0.5), (0.2, 2.0)]]
    W, alpha, beta = max(grid, key=lambda g: sum(clearing(*g)))
    tr.beam.alpha, tr.beam.beta, tr.beam.beam_width = alpha, beta, W
    seen.clear()
    outs = tr.evalute_manifest(man, batch_size=2)
    assert len(outs) == 2 and sum(len(o["pred"]) for o in outs) == 3
    preds = [t for o in outs for t in o["pred"]]
    utts = [(lp_b[i], int(ln[i])) for lp_b, ln in seen for i in range(lp_b.shape[0])]
    checked = 0
    for (u, n_), pred in zip(utts, preds):
        hyps, m, _ = LO.beam_search(u, n_, len(EN_SP), EN_SP, lm, alpha, beta, W, 40, 1.0, 1)
        if m >= margin_min(n_):
            checked += 1
            assert pred == "".join(EN_SP[c] for c in hyps[0][0]), (pred, hyps[0][0])
    assert checked >= 2, checked
    for o in outs:
        assert math.isfinite(float(o["test_loss"]))
        assert float(o["test_wer"]) == pytest.approx(word_error_rate(o["pred"], o["true"], use_cer=tr.model.wer.use_cer), abs=1e-6)
    # the translator without an LM decodes the same audio through the LM-free search
    plain = AsrTranslator(ckpt, map_location="cuda", decoder="beam", beam_width=W)
    assert plain.beam.scorer is None
