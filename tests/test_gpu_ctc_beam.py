"""GPU tier of the CTC prefix beam search (csrc/ctc_beam.hip): n-best lists against the f64 oracle
(tests/helpers/ctc_beam_oracle.py), exactness against brute force on tiny inputs, the likelihood bound at full size,
determinism, graph capture, and the Python surface (BeamSearchDecoderWithLM, AsrTranslator(decoder="beam")).

The kernel computes in f32.  Its choices can only be held to the oracle's where no decision is closer than f32 rounding
can reach, so every oracle comparison first asserts the oracle's margin (smallest relative gap between what a frame kept and
the best of what it dropped) clears margin_min(T) = 8 * 2^-24 * sqrt(T): a random walk of one f32 rounding per frame, eight
times over.  Scores must agree to the same relative tolerance.  Inputs are seeded, peaky log-softmaxed normals (one hot
class per frame, the blank 60 % of the time), as CTC outputs are; where a seed falls short of the margin the next of a
fixed short list is taken, so every case runs."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ctc_beam_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


def margin_min(T: int) -> float:
    return 8.0 * 2.0 ** -24 * math.sqrt(max(int(T), 1))


def peaky(B, T, C, seed, hot=8.0, sd=2.0, p_blank=0.6, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, T, C, generator=g, device=device) * sd
    hotc = torch.randint(0, C - 1, (B, T), generator=g, device=device)
    hotc = torch.where(torch.rand(B, T, generator=g, device=device) < p_blank, torch.full_like(hotc, C - 1), hotc)
    x.scatter_add_(2, hotc.unsqueeze(-1), torch.full((B, T, 1), float(hot), device=device))
    return torch.log_softmax(x, -1)


def oracle_case(B, T, C, W, k, cp, n_best, lens=None, hot=8.0, sd=2.0, seeds=(0, 1, 2, 3, 4, 5, 6, 7)):
    """the first seed whose oracle margin clears margin_min(T): (log-probs (B,T,C) f32 CPU, oracle n-best lists)"""
    worst = 0.0
    for seed in seeds:
        x = peaky(B, T, C, seed, hot, sd)
        res, m = O.beam_search_batch(x.numpy(), lens, C - 1, W, k, cp, n_best)
        if m >= margin_min(T):
            return x, res
        worst = max(worst, m)
    raise AssertionError("no seed of %s gives an oracle margin above %.2e (best %.2e)" % (seeds, margin_min(T), worst))


def run(dev, x, lens, W, k, cp, n_best):
    lt = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    from lightning_asr_amd import ops
    tok, n, sc = ops.ctc_beam_decode(x.to(dev).contiguous(), lt, x.shape[-1] - 1, W, k, cp, n_best)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), n.cpu().numpy(), sc.cpu().numpy()


def assert_matches(got, res, n_best, T):
    tok, n, sc = got
    tol = margin_min(T)
    for b, hyps in enumerate(res):
        for j in range(n_best):
            if j < len(hyps):
                want, ws = hyps[j]
                assert n[b, j] == len(want), (b, j, n[b, j], len(want))
                assert tuple(int(c) for c in tok[b, j, :n[b, j]]) == want, (b, j)
                assert (tok[b, j, n[b, j]:] == -1).all()
                assert abs(sc[b, j] - ws) <= tol * max(1.0, abs(ws)), (b, j, float(sc[b, j]), ws)
            else:
                assert n[b, j] == -1 and sc[b, j] == -np.inf and (tok[b, j] == -1).all(), (b, j)


@pytest.mark.parametrize("W", [1, 4, 16, 64, 128])
@pytest.mark.parametrize("k", [40, 8])
@pytest.mark.parametrize("cp", [1.0, 0.95])
def test_beam_matches_oracle_c28(dev, W, k, cp):
    B, T, C = 3, 50, 28
    n_best = min(W, 4)
    x, res = oracle_case(B, T, C, W, k, cp, n_best)
    assert_matches(run(dev, x, None, W, k, cp, n_best), res, n_best, T)


def test_beam_ragged_lengths(dev):
    B, T, C, W = 6, 40, 28, 16
    lens = [40, 0, 1, 17, 33, 2]
    x, res = oracle_case(B, T, C, W, 40, 1.0, 3, lens=lens)
    got = run(dev, x, lens, W, 40, 1.0, 3)
    assert_matches(got, res, 3, T)
    assert got[1][1, 0] == 0 and got[2][1, 0] == 0.0 and (got[1][1, 1:] == -1).all()   # lens 0: the empty hypothesis, score 0
    # and lens=None is the full length
    x2, res2 = oracle_case(2, 30, C, W, 40, 1.0, 2)
    assert_matches(run(dev, x2, None, W, 40, 1.0, 2), res2, 2, 30)


def test_beam_large_vocabulary(dev):
    """AISHELL-1's vocabulary: C = 4334 takes the radix-select pruning path"""
    B, T, C, W = 4, 400, 4334, 16
    x, res = oracle_case(B, T, C, W, 40, 1.0, 4, hot=16.0, seeds=(0, 1, 2, 3))
    assert_matches(run(dev, x, None, W, 40, 1.0, 4), res, 4, T)


def test_beam_widest_candidate_set(dev):
    """C = 48 keeps cutoff_top_n = 40 classes: beam 128 then has 128 * 41 candidates per frame, the J = 33 search (the widest
    rung), at the smallest vocabulary that reaches it"""
    B, T, C, W, k = 2, 30, 48, 128, 40
    assert W * (k + 1) > 16 * 256
    x, res = oracle_case(B, T, C, W, k, 1.0, 4)
    assert_matches(run(dev, x, None, W, k, 1.0, 4), res, 4, T)


def test_beam_40s_utterance(dev):
    """one 40 s dev clip's worth of frames (T' = 2001) at beam 64"""
    T, C, W = 2001, 28, 64
    x, res = oracle_case(1, T, C, W, 40, 1.0, 4, hot=12.0, seeds=(0,))
    assert_matches(run(dev, x, None, W, 40, 1.0, 4), res, 4, T)


def test_beam_exact_against_brute_force(dev):
    """beam_width >= every distinct prefix and cutoff_top_n = C: the top hypothesis is the most probable labelling and its
    score its log-likelihood (= -F.ctc_loss)"""
    g = torch.Generator().manual_seed(3)
    for T, C in [(5, 3), (4, 4), (3, 4), (1, 3), (6, 2)]:
        for _ in range(3):
            x = torch.log_softmax(torch.randn(1, T, C, generator=g) * 1.5, -1)
            exact = O.brute_force(x[0].double().numpy(), C - 1)
            best = max(exact.items(), key=lambda kv: kv[1])
            tok, n, sc = run(dev, x, None, 128, C, 1.0, 1)
            assert tuple(tok[0, 0, :n[0, 0]]) == best[0]
            tgt = torch.tensor([list(best[0]) or [0]])
            nll = torch.nn.functional.ctc_loss(x.double().transpose(0, 1), tgt, torch.tensor([T]), torch.tensor([len(best[0])]),
                                               blank=C - 1, reduction="none").item()
            assert abs(sc[0, 0] - best[1]) <= 1e-5 * max(1.0, abs(best[1]))
            assert abs(-nll - best[1]) <= 1e-9


def test_beam_scores_bound_full_size(dev):
    """B = 32, T' = 801, C = 4334, beam 64 (too slow for the oracle): every returned score is at most the log-likelihood of its
    hypothesis (ops.ctc_loss), hypotheses are distinct per utterance and come best first"""
    from lightning_asr_amd import ops
    B, T, C, W, nb = 32, 801, 4334, 64, 4
    x = peaky(B, T, C, 11, hot=10.0, device=str(dev)).contiguous()
    lens = torch.randint(600, T + 1, (B,), generator=torch.Generator().manual_seed(4)).to(torch.int32)
    lens[0] = T
    lt = lens.to(dev)
    tok, n, sc = ops.ctc_beam_decode(x, lt, C - 1, W, 40, 1.0, nb)
    tok_h, n_h, sc_h = tok.cpu().numpy(), n.cpu().numpy(), sc.cpu().numpy()
    assert (n_h >= 0).all()
    for b in range(B):
        hyps = [tuple(tok_h[b, j, :n_h[b, j]]) for j in range(nb)]
        assert len(set(hyps)) == nb
        assert all(sc_h[b, j] >= sc_h[b, j + 1] for j in range(nb - 1))
    for j in range(nb):
        S = int(n_h[:, j].max())
        tg = torch.zeros(B, max(S, 1), dtype=torch.int64)
        for b in range(B):
            tg[b, :n_h[b, j]] = torch.from_numpy(tok_h[b, j, :n_h[b, j]].astype(np.int64))
        nll, _ = ops.ctc_loss(x, tg.to(dev), lt, n.new_tensor(n_h[:, j]).to(dev), C - 1, want_grad=False)
        ll = -nll.cpu().numpy()
        tol = 4 * margin_min(T) * np.maximum(1.0, np.abs(ll))
        assert (sc_h[:, j] <= ll + tol).all(), (j, float((sc_h[:, j] - ll).max()))
        assert np.isfinite(ll).all()


def test_beam_deterministic_and_graph_capture(dev):
    from lightning_asr_amd import ops
    B, T, C = 8, 200, 28
    x = peaky(B, T, C, 5, device=str(dev)).contiguous()
    lens = torch.tensor([200, 150, 1, 0, 199, 77, 120, 200], dtype=torch.int32, device=dev)
    a = ops.ctc_beam_decode(x, lens, C - 1, 32, 40, 0.95, 8)
    b = ops.ctc_beam_decode(x, lens, C - 1, 32, 40, 0.95, 8)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.ctc_beam_decode(x, lens, C - 1, 32, 40, 0.95, 8)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = ops.ctc_beam_decode(x, lens, C - 1, 32, 40, 0.95, 8)
    g.replay()
    torch.cuda.synchronize()
    for u, v in zip(a, c):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------ Python surface
def test_decoder_with_lm_surface(dev):
    from lightning_asr_amd.beam_search import BeamSearchDecoderWithLM
    from lightning_asr_amd.predict import EN_LABELS
    C = len(EN_LABELS) + 1
    x, res = oracle_case(3, 60, C, 16, 40, 1.0, 3, lens=[60, 45, 12])
    want = ["".join(EN_LABELS[c] for c in r[0][0]) for r in res]
    dec = BeamSearchDecoderWithLM(EN_LABELS, 16, 1.0, 1.0, None, 4, cutoff_prob=1.0, cutoff_top_n=40)
    assert dec.forward(x.numpy(), np.array([60, 45, 12])) == want
    assert dec(x.to(dev), torch.tensor([60, 45, 12], device=dev)) == want
    nbest = dec.decode_nbest(x.numpy(), [60, 45, 12], 3)
    for b, r in enumerate(res):
        assert [t for _, t in nbest[b]] == ["".join(EN_LABELS[c] for c in p) for p, _ in r]
        assert all(abs(s - ws) <= margin_min(60) * max(1, abs(ws)) for (s, _), (_, ws) in zip(nbest[b], r))


def _translator_fixture(tmp_path):
    import wave as wavmod
    from oracle import ref_cpu as R
    from lightning_asr_amd.predict import EN_LABELS
    state = R.formula_state("plain", 29)
    for k_ in state:
        if k_.endswith("running_var"):
            state[k_] = state[k_] * 0 + 0.5 + 0.01 * torch.arange(state[k_].numel()).float() % 1.0
    ckpt = {"state_dict": {"encoder." + k_: v for k_, v in state.items()},
            "hyper_parameters": {"learning_rate": 1e-2, "weight_decay": 1e-3, "labels": EN_LABELS, "total_epoch": 1, "drop_rate": 0.0,
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


def test_translator_beam_matches_oracle(dev, tmp_path):
    from lightning_asr_amd.predict import AsrTranslator, EN_LABELS
    ckpt, wavs, _ = _translator_fixture(tmp_path)
    W = 4
    tr = AsrTranslator(ckpt, map_location="cuda", decoder="beam", beam_width=W, cutoff_top_n=40)
    wp = wavs[0][0]
    dith = tr.audio_parser.device_dither()
    step0 = dith.step.clone()
    text = tr.translate(wp)
    dith.step.copy_(step0)                       # the same dither draw again: the same features and log-probs
    inputs = tr.audio_parser.parse_audio(wp, mask=False)
    with torch.no_grad():
        lp = tr.model._encode(inputs, torch.ones(1, device=dev)).float().cpu().numpy()
    res, m = O.beam_search_batch(lp, None, len(EN_LABELS), W, 40, 1.0, 3)
    assert m >= margin_min(lp.shape[1]), m
    assert text == "".join(EN_LABELS[c] for c in res[0][0][0])
    dith.step.copy_(step0)
    nb = tr.translate_nbest(wp, 3)
    assert [t for t, _ in nb] == ["".join(EN_LABELS[c] for c in p) for p, _ in res[0]]


def test_evaluate_manifest_beam_and_greedy(dev, tmp_path):
    from lightning_asr_amd.predict import AsrTranslator
    from lightning_asr_amd.utils.asr_metrics import word_error_rate
    ckpt, wavs, man = _translator_fixture(tmp_path)
    tr = AsrTranslator(ckpt, map_location="cuda", decoder="beam", beam_width=8)
    outs = tr.evalute_manifest(man, batch_size=2)
    assert len(outs) == 2 and sum(len(o["pred"]) for o in outs) == 3
    for o in outs:
        assert set(o) == {"test_loss", "input", "test_wer", "pred", "true", "path"}
        assert math.isfinite(float(o["test_loss"]))
        assert float(o["test_wer"]) == pytest.approx(word_error_rate(o["pred"], o["true"], use_cer=tr.model.wer.use_cer), abs=1e-6)
    # greedy stays the Trainer.test path: the default translator and decoder="greedy" agree with what test_step returns
    g = AsrTranslator(ckpt, map_location="cuda")
    assert g.decoder == "greedy"
    outs_g = g.evalute_manifest(man, batch_size=2)
    outs_g2 = tr.evalute_manifest(man, batch_size=2, decoder="greedy")
    assert [o["true"] for o in outs_g] == [o["true"] for o in outs]
    assert [o["pred"] for o in outs_g] == [o["pred"] for o in outs_g2]
    assert isinstance(g.translate(wavs[0][0]), str)
