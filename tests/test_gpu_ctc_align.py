"""GPU tier of CTC forced alignment (csrc/ctc_align.hip).  The recursion is a max and one f32 add per state per frame, so the
kernel is held to the numpy oracle (tests/helpers/ctc_align_oracle.py) BIT FOR BIT: scores, frame states, frame log-probs and
label spans, across every lattice geometry (4 / 8 / 16 states per lane, 2..4 waves), both emission paths (LDS block, register
ring) and both homes of the backpointer table (LDS, workspace).  Then: infeasible rows among feasible ones, guard bands round
every output and the workspace, consistency with ops.ctc_loss, graph capture, and the Python surface of AsrTranslator."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ctc_align_oracle as A  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("score", "frame_state", "frame_logp", "label_start", "label_end")


def peaky(B, T, C, seed, hot=8.0, sd=2.0, p_blank=0.6):
    """the generator of the beam tests: one hot class per frame, the blank 60 % of the time"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g) * sd
    hotc = torch.randint(0, C - 1, (B, T), generator=g)
    hotc = torch.where(torch.rand(B, T, generator=g) < p_blank, torch.full_like(hotc, C - 1), hotc)
    x.scatter_add_(2, hotc.unsqueeze(-1), torch.full((B, T, 1), float(hot)))
    return torch.log_softmax(x, -1)


def plain(B, T, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, T, C, generator=g) * 2.0, -1)


def n_repeats(t):
    return sum(1 for a, b in zip(t, t[1:]) if a == b)


def make_case(S_max, T, C, seed, B=4):
    """ragged batch over a (B, S_max) target block: row 0 as long as S_max and T allow (feasible), row 1 without labels, row 2
    with in_lens 0, the rest random; labels from a small alphabet so that runs of equal labels are common"""
    rng = np.random.RandomState(seed)
    alphabet = min(C - 1, 4)
    targets = rng.randint(0, alphabet, size=(B, S_max)).astype(np.int64)
    in_lens = np.full(B, T, np.int32)
    tgt_lens = np.zeros(B, np.int32)
    for b in range(B):
        if b == 1:
            tgt_lens[b], in_lens[b] = 0, max(T - 1, 0)
            continue
        if b == 2:
            tgt_lens[b], in_lens[b] = min(S_max, 3), 0
            continue
        Tb = T if b == 0 else int(rng.randint(max(T // 2, 1), T + 1))
        S = S_max if b == 0 else int(rng.randint(0, S_max + 1))
        while S > 0 and S + n_repeats(targets[b, :S].tolist()) > Tb:      # shrink to the longest feasible prefix
            S -= 1
        in_lens[b], tgt_lens[b] = Tb, S
    return targets, in_lens, tgt_lens


def run_ops(dev, lp, targets, in_lens, tgt_lens, blank):
    from lightning_asr_amd import ops
    out = ops.ctc_align(lp.to(dev).contiguous(), torch.from_numpy(targets).to(dev),
                        None if in_lens is None else torch.from_numpy(in_lens).to(dev), torch.from_numpy(tgt_lens).to(dev), blank)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def assert_exact(got, want, ctx):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (ctx, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %d places, first %s: got %r want %r"
                                 % (ctx, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


# every geometry boundary of ctc_geom (127|128: 4 -> 8 states per lane, 255|256: 8 -> 16, 511|512: one wave -> two, 1023: two,
# 1500: three, 2047: four), the shortest clips, and T' = 501 / 2001 where the backpointer table leaves LDS for the workspace
CASES_C28 = [(0, 1), (0, 50), (1, 1), (1, 2), (1, 50), (127, 2), (127, 50), (127, 501), (128, 501), (255, 501), (256, 501),
             (256, 50), (511, 2001), (512, 2001), (512, 50), (1023, 2001), (1500, 2001), (2047, 2001), (2047, 50)]
CASES_C4334 = [(0, 2), (1, 50), (127, 501), (128, 50), (256, 501), (511, 501), (512, 501), (1500, 2001), (2047, 50)]


@pytest.mark.parametrize("S_max,T", CASES_C28)
@pytest.mark.parametrize("gen", ["plain", "peaky"])
def test_align_matches_oracle_c28(dev, S_max, T, gen):
    C = 28
    lp = (plain if gen == "plain" else peaky)(4, T, C, 100 + S_max + T)
    targets, in_lens, tgt_lens = make_case(S_max, T, C, 7 + S_max + T)
    want = A.align_batch(lp.numpy(), targets, in_lens, tgt_lens, C - 1)
    assert np.isfinite(want[0][0]) and want[0][2] == (0.0 if tgt_lens[2] == 0 else -np.inf)
    assert_exact(run_ops(dev, lp, targets, in_lens, tgt_lens, C - 1), want, (S_max, T, gen))


@pytest.mark.parametrize("S_max,T", CASES_C4334)
def test_align_matches_oracle_c4334(dev, S_max, T):
    """AISHELL-1's vocabulary: the emission block does not fit LDS, the recursion runs on the register ring"""
    C, B = 4334, 3
    gen = peaky if (S_max + T) % 2 else plain
    lp = gen(B, T, C, 300 + S_max + T)
    targets, in_lens, tgt_lens = make_case(S_max, T, C, 11 + S_max + T, B=B)
    want = A.align_batch(lp.numpy(), targets, in_lens, tgt_lens, C - 1)
    assert np.isfinite(want[0][0])
    assert_exact(run_ops(dev, lp, targets, in_lens, tgt_lens, C - 1), want, (S_max, T))


def test_align_in_lens_none_and_blank_not_last(dev):
    """in_lens = None means T; the blank may be any class; out-of-range lengths are clamped on the device"""
    C, T, S_max = 28, 60, 9
    lp = plain(3, T, C, 5)
    rng = np.random.RandomState(3)
    targets = rng.randint(1, C, size=(3, S_max)).astype(np.int64)
    tgt_lens = np.array([9, 4, 0], np.int32)
    want = A.align_batch(lp.numpy(), targets, None, tgt_lens, 0)
    assert_exact(run_ops(dev, lp, targets, None, tgt_lens, 0), want, "in_lens=None, blank=0")
    in_lens = np.array([T + 100, -5, 17], np.int32)
    tl2 = np.array([S_max + 50, 2, -3], np.int32)
    want = A.align_batch(lp.numpy(), targets, in_lens, tl2, 0)
    assert_exact(run_ops(dev, lp, targets, in_lens, tl2, 0), want, "clamped lengths")
    assert (want[1][1] == -1).all() and want[0][1] == -np.inf and want[1][0, T - 1] >= 0


def test_align_infeasible_rows_among_feasible(dev):
    C, T, S_max, blank = 28, 40, 12, 27
    lp = peaky(6, T, C, 21).clone()
    targets = np.array([[1, 2, 2, 3, 3, 3, 4, 5, 5, 6, 7, 8]] * 6, np.int64)
    rep = n_repeats(targets[0].tolist())
    in_lens = np.array([T, S_max + rep - 1, S_max + rep, T, T, T], np.int32)   # row 1: one frame short; row 2: exactly enough
    tgt_lens = np.full(6, S_max, np.int32)
    lp[3, 10, :] = -np.inf                      # row 3: every path crosses a frame of -inf emissions
    lp[4, :, 5] = -np.inf                       # row 4: label 5 can never be emitted
    lp[5, 3:20, 9] = -np.inf                    # row 5: -inf on a class the target does not use, and on the blank in a few frames
    lp[5, 25:28, blank] = -np.inf
    want = A.align_batch(lp.numpy(), targets, in_lens, tgt_lens, blank)
    assert [bool(np.isfinite(s)) for s in want[0]] == [True, False, True, False, False, True]
    got = run_ops(dev, lp, targets, in_lens, tgt_lens, blank)
    assert_exact(got, want, "infeasible mix")
    for b in (1, 3, 4):
        assert got[0][b] == -np.inf and (got[1][b] == -1).all() and (got[2][b] == 0).all()
        assert (got[3][b] == -1).all() and (got[4][b] == -1).all()
    # the tight row uses every frame: no blank between different labels, one between equal ones
    assert (got[1][2, :in_lens[2]] >= 0).all() and got[3][2, 0] == 0 and got[4][2, S_max - 1] == in_lens[2]


def test_align_guard_bands_and_fills(dev):
    """every output and the workspace sit between sentinel regions that must come back intact; rows past in_lens and labels past
    tgt_lens hold exactly the documented fill"""
    from lightning_asr_amd import _lib
    G = 1024                                                        # guard elements on either side
    for S_max, T, C in [(40, 120, 28), (300, 501, 28), (600, 700, 28), (40, 64, 4334)]:
        B = 3
        lp = plain(B, T, C, S_max).to(dev).contiguous()
        targets, in_lens, tgt_lens = make_case(S_max, T, C, S_max + 1, B=B)
        tg, il, tl = torch.from_numpy(targets).to(dev), torch.from_numpy(in_lens).to(dev), torch.from_numpy(tgt_lens).to(dev)
        nb = int(_lib.load().lasr_ctc_align_workspace_bytes(B, T, S_max))
        assert nb > 0 and nb % 4 == 0
        sizes = {"score": B, "frame_state": B * T, "frame_logp": B * T, "label_start": B * S_max, "label_end": B * S_max, "ws": nb // 4}
        bufs = {k: torch.full((n + 2 * G,), -12345, dtype=torch.int32, device=dev) for k, n in sizes.items()}
        ptr = {k: v.data_ptr() + 4 * G for k, v in bufs.items()}
        _lib.call("lasr_ctc_align", lp.data_ptr(), tg.data_ptr(), il.data_ptr(), tl.data_ptr(), B, T, C, S_max, C - 1, ptr["score"],
                  ptr["frame_state"], ptr["frame_logp"], ptr["label_start"], ptr["label_end"], ptr["ws"], nb,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for k, v in bufs.items():
            h = v.cpu().numpy()
            assert (h[:G] == -12345).all() and (h[G + sizes[k]:] == -12345).all(), (S_max, T, C, k)
        body = {k: bufs[k].cpu().numpy()[G:G + sizes[k]] for k in sizes}
        got = (body["score"].view(np.float32), body["frame_state"].reshape(B, T), body["frame_logp"].view(np.float32).reshape(B, T),
               body["label_start"].reshape(B, S_max), body["label_end"].reshape(B, S_max))
        want = A.align_batch(lp.cpu().numpy(), targets, in_lens, tgt_lens, C - 1)
        assert_exact(got, want, ("guard", S_max, T, C))
        for b in range(B):
            Tb, S = int(in_lens[b]), int(tgt_lens[b])
            assert (got[1][b, Tb:] == -1).all() and (got[2][b, Tb:] == 0).all()
            assert (got[3][b, S:] == -1).all() and (got[4][b, S:] == -1).all()
            if np.isfinite(got[0][b]):
                assert (got[1][b, :Tb] >= 0).all() and (got[3][b, :S] >= 0).all() and (got[4][b, :S] > got[3][b, :S]).all()


def test_align_consistent_with_loss(dev):
    """the best path is one term of the likelihood: score <= -nll + 1e-4 * max(1, |nll|) (1e-4: the loss's documented accuracy);
    the frame log-probs of the path sum to the score (f32 summation error: T * 2^-24 relative, sum taken in f64); the path
    collapses to the target"""
    from lightning_asr_amd import ops
    for S_max, T, C, B in [(100, 501, 28, 8), (600, 2001, 28, 2), (60, 300, 4334, 3)]:
        lp = peaky(B, T, C, 40 + S_max).to(dev).contiguous()
        targets, in_lens, tgt_lens = make_case(S_max, T, C, 50 + S_max, B=B)
        tg, il, tl = torch.from_numpy(targets).to(dev), torch.from_numpy(in_lens).to(dev), torch.from_numpy(tgt_lens).to(dev)
        al = ops.ctc_align(lp, tg, il, tl, C - 1)
        il1 = il.clamp(min=1)                                                # the loss is not defined for in_lens 0: those rows are skipped below
        nll, _ = ops.ctc_loss(lp, tg, il1, tl, C - 1, want_grad=False)
        score, st, flp = al.score.cpu().numpy(), al.frame_state.cpu().numpy(), al.frame_logp.cpu().numpy()
        nll = nll.cpu().numpy()
        n_checked = 0
        for b in range(B):
            Tb, S = int(in_lens[b]), int(tgt_lens[b])
            if Tb == 0:
                continue
            n_checked += 1
            assert np.isfinite(score[b]) and np.isfinite(nll[b])
            print("consistency S_max=%d T=%d C=%d b=%d: score %.6f  -nll %.6f" % (S_max, T, C, b, score[b], -nll[b]))
            assert score[b] <= -nll[b] + 1e-4 * max(1.0, abs(nll[b])), (b, score[b], -nll[b])
            total = float(flp[b, :Tb].astype(np.float64).sum())
            assert abs(total - float(score[b])) <= Tb * 2.0 ** -24 * max(1.0, abs(float(score[b]))), (b, total, score[b])
            tgt = targets[b, :S].tolist()
            assert A.valid_path(st[b, :Tb], S) and A.collapse(st[b, :Tb].tolist(), tgt, C - 1) == tgt
        assert n_checked >= 2


def test_align_deterministic_and_graph_capture(dev):
    from lightning_asr_amd import ops
    for S_max, T, C in [(150, 501, 28), (600, 800, 28)]:
        B = 4
        lp = peaky(B, T, C, 5).to(dev).contiguous()
        targets, in_lens, tgt_lens = make_case(S_max, T, C, 9, B=B)
        tg, il, tl = torch.from_numpy(targets).to(dev), torch.from_numpy(in_lens).to(dev), torch.from_numpy(tgt_lens).to(dev)
        a = ops.ctc_align(lp, tg, il, tl, C - 1)
        b = ops.ctc_align(lp, tg, il, tl, C - 1)
        torch.cuda.synchronize()
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.ctc_align(lp, tg, il, tl, C - 1)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c = ops.ctc_align(lp, tg, il, tl, C - 1)
        for _ in range(2):
            for o in c:
                o.fill_(-7)
            g.replay()
            torch.cuda.synchronize()
            for u, v in zip(a, c):
                assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------ Python surface
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
    return str(path), wavs


def test_translator_align_matches_oracle(dev, tmp_path):
    from lightning_asr_amd.align import unit_records
    from lightning_asr_amd.predict import AsrTranslator, EN_LABELS
    ckpt, wavs = _translator_fixture(tmp_path)
    tr = AsrTranslator(ckpt, map_location="cuda")
    assert tr.frame_seconds() == pytest.approx(0.02)                # 160 samples at 16 kHz, time stride 2
    wp, secs = wavs[0]
    dith = tr.audio_parser.device_dither()
    step0 = dith.step.clone()
    words = tr.align(wp, "hello world")
    assert [w["word"] for w in words] == ["hello", "world"]
    assert ["".join(r["label"] for r in w["labels"]) for w in words] == ["hello", "world"]
    flat = [r for w in words for r in w["labels"]]
    for r in flat + words:
        assert 0.0 <= r["start"] < r["end"] <= secs and 0.0 < r["score"] <= 1.0
    for a, b in zip(flat, flat[1:]):
        assert a["end"] <= b["start"]
    assert words[0]["end"] <= words[1]["start"]
    # the same dither draw again: the same features and log-probs, through the oracle and the pure functions
    dith.step.copy_(step0)
    inputs = tr.audio_parser.parse_audio(wp, mask=False)
    with torch.no_grad():
        lp = tr.model._encode(inputs, torch.ones(1, device=dev)).float().cpu().numpy()
    ids = [EN_LABELS.index(c) for c in "hello world"]
    score, st, flp, ls, le = A.align_batch(lp, [ids], None, [len(ids)], len(EN_LABELS))
    assert np.isfinite(score[0])
    assert words == unit_records(ids, ls[0].tolist(), le[0].tolist(), flp[0].tolist(), EN_LABELS, 0.02, secs)
    with pytest.raises(ValueError, match="é"):
        tr.align(wp, "héllo")
    with pytest.raises(ValueError, match="too long"):
        tr.align(wp, "ab" * 100)                                    # 200 labels on ~100 frames
    assert tr.align(wp, "") == []


@pytest.mark.parametrize("decoder", ["greedy", "beam"])
def test_translate_timed_matches_translate(dev, tmp_path, decoder):
    from lightning_asr_amd.predict import AsrTranslator
    ckpt, wavs = _translator_fixture(tmp_path)
    tr = AsrTranslator(ckpt, map_location="cuda", decoder=decoder, beam_width=8)
    dith = tr.audio_parser.device_dither()
    for wp, secs in wavs[:2]:
        step0 = dith.step.clone()
        text = tr.translate(wp)
        dith.step.copy_(step0)
        text2, words = tr.translate_timed(wp)
        assert text2 == text
        assert [w["word"] for w in words] == text.split()
        if not text:
            assert words == []
        for w in words:
            assert 0.0 <= w["start"] < w["end"] <= secs
        for a, b in zip(words, words[1:]):
            assert a["end"] <= b["start"]


def test_align_manifest_marks_infeasible_lines(dev, tmp_path):
    from lightning_asr_amd.predict import AsrTranslator
    ckpt, wavs = _translator_fixture(tmp_path)
    texts = ("a b", "ab" * 60, "it's a test")                      # line 2: 120 labels on the ~76 frames of a 1.5 s clip
    man = tmp_path / "m.json"
    with open(man, "w") as f:
        for (wp, secs), text in zip(wavs, texts):
            f.write(json.dumps({"audio_filepath": wp, "duration": secs, "text": text}) + "\n")
    tr = AsrTranslator(ckpt, map_location="cuda")
    out_path = tmp_path / "aligned.jsonl"
    recs = tr.align_manifest(str(man), str(out_path), batch_size=2)
    lines = [json.loads(l) for l in open(out_path, encoding="utf-8") if l.strip()]
    assert len(recs) == 3 and len(lines) == 3
    by_path = {r["audio_filepath"]: r for r in lines}
    for (wp, secs), text in zip(wavs, texts):
        r = by_path[wp]
        assert set(r) == {"audio_filepath", "text", "score", "score_per_frame", "words"} and r["text"] == text
        if text == texts[1]:
            assert r["words"] is None and r["score"] == -math.inf
        else:
            assert math.isfinite(r["score"]) and r["score"] < 0 and math.isfinite(r["score_per_frame"])
            assert [w["word"] for w in r["words"]] == text.split()
            assert all(0.0 <= w["start"] < w["end"] <= secs for w in r["words"])
    assert [json.loads(json.dumps(r)) for r in recs] == lines
