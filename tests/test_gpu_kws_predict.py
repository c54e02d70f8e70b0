"""GPU tier of the keyword-search surface of ``AsrTranslator``: ``find_keywords``, ``keyword_scores`` and ``find_keywords_long``
against the numpy oracle (tests/helpers/kws_oracle.py) and the pure record functions of lightning_asr_amd/kws.py on the same
log-probs.  Formula-state checkpoint and synthetic wavs, as tests/test_gpu_ctc_align.py; the same dither draw is had again by
resetting the device dither's step."""
import math
import os
import sys
import wave as wavmod

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kws_oracle as K  # noqa: E402

pytestmark = pytest.mark.gpu

KEYWORDS = ["hello", "a", "to you", "hello"]          # a word, one label, a phrase with a space, a duplicate
# Formula weights give log-probs that follow no text, so the thresholds here are loose ones that let spans through; what is
# checked is that the surface reports exactly what the definition gives on the model's own log-probs.
THRESHOLDS = (-2.0, -4.0, -50.0)
MAX_HITS = 256                                         # above the frames of any clip here: no pair can overflow


def _clip(i, secs):
    g = torch.Generator().manual_seed(5 + i)
    n = int(16000 * secs)
    t = torch.arange(n) / 16000.0
    y = 0.3 * torch.sin(2 * math.pi * (220 + 60 * i + 180 * t) * t) + 0.05 * torch.randn(n, generator=g)
    return (y.clamp(-1, 1) * 32767).to(torch.int16).numpy()


def _write_wav(path, pcm):
    with wavmod.open(str(path), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000); f.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    from oracle import ref_cpu as R
    from lightning_asr_amd.predict import AsrTranslator, EN_LABELS
    d = tmp_path_factory.mktemp("kws")
    state = R.formula_state("plain", 29)
    for k_ in state:
        if k_.endswith("running_var"):
            state[k_] = state[k_] * 0 + 0.5 + 0.01 * torch.arange(state[k_].numel()).float() % 1.0
    ckpt = {"state_dict": {"encoder." + k_: v for k_, v in state.items()},
            "hyper_parameters": {"learning_rate": 1e-2, "weight_decay": 1e-3, "labels": EN_LABELS, "total_epoch": 1, "drop_rate": 0.0,
                                 "mask": True, "use_cer": False}, "epoch": 0, "global_step": 0}
    torch.save(ckpt, d / "ref_style.ckpt")
    a, b = _clip(0, 2.0), _clip(1, 1.5)
    _write_wav(d / "a0.wav", a)
    # two clips with 1.5 s of silence between them, half a second before and after
    _write_wav(d / "rec.wav", np.concatenate([np.zeros(8000, np.int16), a, np.zeros(24000, np.int16), b, np.zeros(8000, np.int16)]))
    tr = AsrTranslator(str(d / "ref_style.ckpt"), map_location="cuda")
    ids = [[EN_LABELS.index(c) for c in k] for k in KEYWORDS]
    return {"dir": d, "tr": tr, "ids": ids, "labels": [c for p in ids for c in p],
            "offsets": np.concatenate([[0], np.cumsum([len(p) for p in ids])]), "lengths": [len(p) for p in ids]}


def _file_logp(world, dev, path):
    """the log-probs find_keywords sees for the file, given the same dither step"""
    tr = world["tr"]
    inputs = tr.audio_parser.parse_audio(path, mask=False)
    with torch.no_grad():
        return tr.model._encode(inputs, torch.ones(1, device=dev)).float().cpu().numpy()


def test_find_keywords_matches_oracle_and_records(world, dev):
    from lightning_asr_amd import kws
    tr, wp = world["tr"], str(world["dir"] / "a0.wav")
    dith = tr.audio_parser.device_dither()
    step0 = dith.step.clone()
    lp = _file_logp(world, dev, wp)
    assert lp.shape[0] == 1 and lp.shape[2] == 29
    n_total = 0
    for thr in THRESHOLDS:
        dith.step.copy_(step0)
        got = tr.find_keywords(wp, KEYWORDS, threshold=thr, max_hits=MAX_HITS)
        n_hits, span, score, _, _ = K.search_batch(lp, None, 28, world["labels"], world["offsets"], max(world["lengths"]), thr, MAX_HITS)
        want = kws.hit_records(KEYWORDS, world["lengths"], n_hits[0].tolist(), span[0].tolist(), score[0].tolist(), 0.02, 2.0)
        assert got == want, thr
        assert [r["start"] for r in got] == sorted(r["start"] for r in got)                # sorted by start
        for r in got:
            assert set(r) == {"keyword", "start", "end", "score", "score_per_label", "confidence"}
            assert 0.0 <= r["start"] <= r["end"] <= 2.0 and r["score"] <= 0.0 and 0.0 < r["confidence"] <= 1.0   # equal: the last frame, clipped
            assert r["score_per_label"] >= thr
        by_kw = {k: [(r["start"], r["end"], r["score"]) for r in got if r["keyword"] == k] for k in KEYWORDS}
        assert len(by_kw["hello"]) == 2 * int(n_hits[0, 0]) and n_hits[0, 0] == n_hits[0, 3]   # the duplicate reports the same hits
        n_total += len(got)
    assert n_total > 0 and len(got) >= 3                    # at -50 per label every keyword that fits the clip has a hit
    # the default threshold is ops.ctc_keyword_search's
    dith.step.copy_(step0)
    assert tr.find_keywords(wp, KEYWORDS, max_hits=MAX_HITS) == tr_default(world, lp)
    with pytest.raises(ValueError, match="é"):
        tr.find_keywords(wp, ["héllo"])
    with pytest.raises(ValueError):
        tr.find_keywords(wp, ["ok", ""])
    with pytest.raises(ValueError):
        tr.find_keywords(wp, [])
    with pytest.raises(TypeError):
        tr.find_keywords(wp, "hello")


def tr_default(world, lp):
    from lightning_asr_amd import kws
    n_hits, span, score, _, _ = K.search_batch(lp, None, 28, world["labels"], world["offsets"], max(world["lengths"]), -2.0, MAX_HITS)
    return kws.hit_records(KEYWORDS, world["lengths"], n_hits[0].tolist(), span[0].tolist(), score[0].tolist(), 0.02, 2.0)


def test_find_keywords_with_the_beam_decoder_setting(world, dev):
    from lightning_asr_amd.predict import AsrTranslator
    tr, wp = world["tr"], str(world["dir"] / "a0.wav")
    tb = AsrTranslator(str(world["dir"] / "ref_style.ckpt"), map_location="cuda", decoder="beam", beam_width=4)
    d0, d1 = tr.audio_parser.device_dither(), tb.audio_parser.device_dither()
    s0, s1 = d0.step.clone(), d1.step.clone()
    d1.step.copy_(s0)                                        # the same dither draw in both translators
    a = tr.find_keywords(wp, KEYWORDS, threshold=-50.0, max_hits=MAX_HITS)
    b = tb.find_keywords(wp, KEYWORDS, threshold=-50.0, max_hits=MAX_HITS)
    d0.step.copy_(s0)
    d1.step.copy_(s1)
    assert a == b and len(a) >= 3


def test_keyword_scores_match_the_oracles_best(world, dev):
    tr, wp = world["tr"], str(world["dir"] / "a0.wav")
    dith = tr.audio_parser.device_dither()
    step0 = dith.step.clone()
    lp = _file_logp(world, dev, wp)
    dith.step.copy_(step0)
    kw = KEYWORDS + ["ab" * 30]                              # 60 labels on ~100 frames fit; see the last assertion for one that does not
    got = tr.keyword_scores(wp, kw)
    ids = world["ids"] + [tr.text_to_ids("ab" * 30)]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in ids])])
    _, _, _, best, bspan = K.search_batch(lp, None, 28, [c for p in ids for c in p], offsets, 60, 0.0, 1)
    assert [r["keyword"] for r in got] == kw
    for k, r in enumerate(got):
        assert np.isfinite(best[0, k]) and r["score_per_label"] == float(best[0, k]) / len(ids[k]), (k, r)
        assert r["start"] == min(int(bspan[0, k, 0]) * 0.02, 2.0) and r["end"] == min(int(bspan[0, k, 1]) * 0.02, 2.0)
    # a threshold at a keyword's score reports it: its best span is a hit
    dith.step.copy_(step0)
    thr = float(np.nextafter(np.float32(got[0]["score_per_label"]), np.float32(-np.inf)))
    hits = tr.find_keywords(wp, ["hello"], threshold=thr, max_hits=MAX_HITS)
    assert any(h["score_per_label"] == got[0]["score_per_label"] for h in hits)
    dith.step.copy_(step0)
    dead = tr.keyword_scores(wp, ["a" * 64])                 # 64 equal labels need 127 frames; the 2 s clip has about 100
    assert lp.shape[1] < 127 and dead == [{"keyword": "a" * 64, "score_per_label": -math.inf, "start": None, "end": None}]
    with pytest.raises(ValueError):
        tr.keyword_scores(wp, ["a" * 65])                    # over KWS_MAX_LABELS


def test_find_keywords_long_offsets_and_segments(world, dev):
    from lightning_asr_amd import kws, ops
    from lightning_asr_amd.data_module import load_wav
    tr, wp = world["tr"], str(world["dir"] / "rec.wav")
    dith = tr.audio_parser.device_dither()
    step0 = dith.step.clone()
    wave = load_wav(wp)[0].to(dev).contiguous()
    found = ops.vad_segments(wave)
    n = int(found.n_segs)
    segs = [tuple(s) for s in found.segs[:n].tolist()]
    assert n == 2 and segs[0][1] < 8000 + 32000 + 12000 < segs[1][0]          # one segment per clip, the silence between them
    order = sorted(range(n), key=lambda i: segs[i][0] - segs[i][1])
    batch = [segs[i] for i in order]
    with torch.no_grad():
        out, t_lens = tr._segment_batch(wave, batch)
    lp, t_lens = out.float().cpu().numpy(), t_lens.tolist()
    for thr in (-4.0, -50.0):
        dith.step.copy_(step0)
        got = tr.find_keywords_long(wp, KEYWORDS, threshold=thr, max_hits=MAX_HITS)
        n_hits, span, score, _, _ = K.search_batch(lp, t_lens, 28, world["labels"], world["offsets"], max(world["lengths"]), thr, MAX_HITS)
        want = []
        for b, (s0, s1) in enumerate(batch):                                   # per-segment oracle runs, moved to the recording's time
            t0, t1 = s0 / 16000.0, s1 / 16000.0
            for r in kws.hit_records(KEYWORDS, world["lengths"], n_hits[b].tolist(), span[b].tolist(), score[b].tolist(), 0.02, t1 - t0):
                r["start"], r["end"] = min(r["start"] + t0, t1), min(r["end"] + t0, t1)
                want.append(r)
        assert got == kws.sort_records(want, KEYWORDS), thr
        keys = [(r["start"], KEYWORDS.index(r["keyword"])) for r in got]
        assert keys == sorted(keys)
        for r in got:                                                          # every hit lies inside a VAD segment
            assert any(s0 / 16000.0 <= r["start"] <= r["end"] <= s1 / 16000.0 for s0, s1 in segs), r
    assert len(got) >= 6 and {r["keyword"] for r in got} == set(KEYWORDS)
    assert any(r["start"] >= segs[1][0] / 16000.0 for r in got) and any(r["end"] <= segs[0][1] / 16000.0 for r in got)
    # more hits of a pair than slots is an error that names the keyword (one-label keywords make many short hits at -50)
    assert int(n_hits[:, 1].max()) > 1
    dith.step.copy_(step0)
    with pytest.raises(ValueError, match=r"'a'.*max_hits=1"):
        tr.find_keywords_long(wp, ["a"], threshold=-50.0, max_hits=1)
    with pytest.raises(ValueError, match="max_segments=1"):
        tr.find_keywords_long(wp, KEYWORDS, max_segments=1)
    dith.step.copy_(step0)
    one = tr.find_keywords_long(wp, KEYWORDS, threshold=-50.0, max_hits=MAX_HITS, batch_size=1)
    # one segment per batch: each batch draws its own dither, so only the shape of the answer is compared
    assert {r["keyword"] for r in one} == set(KEYWORDS)
    assert all(any(s0 / 16000.0 <= r["start"] <= r["end"] <= s1 / 16000.0 for s0, s1 in segs) for r in one)
    with pytest.raises(ValueError):
        tr.find_keywords_long(wp, KEYWORDS, batch_size=0)
