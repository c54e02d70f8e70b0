"""AsrTranslator.encode_long / align_long / cut_corpus on the GPU, with a formula-weight checkpoint and a synthetic
recording of 60 s (as tests/test_gpu_streaming.py builds its own): the batched whole-recording encoder against the streaming
recogniser's rows, the banded alignment of the model's own greedy hypothesis, and the corpus cutter's wavs and manifest."""
import json
import math
import os
import sys
import wave as wavmod

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ctc_align_oracle as A  # noqa: E402

pytestmark = pytest.mark.gpu

SECS = 60.0
WIN = dict(window_s=8.0, context_s=2.0)
# max |logp(batch_size=4) - logp(batch_size=1)| over the recording, measured on an MI355X (DESIGN.md "Long-recording forced
# alignment"): 0.0 - the forward's kernels gave the same bits for a batch of four equal-length windows as for each on its own.
# The gate is 2 x the measurement.
BATCH_DIFF_MEASURED = 0.0


def synth_wave(secs, seed=5):
    g = torch.Generator().manual_seed(seed)
    n = int(16000 * secs)
    t = torch.arange(n) / 16000.0
    y = 0.3 * torch.sin(2 * math.pi * (220 + 180 * (t % 3.0)) * t) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3.0 * t)) \
        + 0.05 * torch.randn(n, generator=g)
    return y.clamp(-1, 1).contiguous()


@pytest.fixture(scope="module")
def setup(dev, tmp_path_factory):
    """the translator, the recording as PCM16 (tensor and file), and its log-probs at batch_size 1 - made once, never written to"""
    from oracle import ref_cpu as R
    from lightning_asr_amd.predict import AsrTranslator, EN_LABELS
    state = R.formula_state("plain", 29, gain=3.0)         # gain 1 decodes every frame as one label; at 3 the hypothesis has ~6 labels a second
    for k_ in state:
        if k_.endswith("running_var"):
            state[k_] = state[k_] * 0 + 0.5 + 0.01 * torch.arange(state[k_].numel()).float() % 1.0
    ck = {"state_dict": {"encoder." + k_: v for k_, v in state.items()},
          "hyper_parameters": {"learning_rate": 1e-2, "weight_decay": 1e-3, "labels": EN_LABELS, "total_epoch": 1, "drop_rate": 0.0,
                               "mask": True, "use_cer": False}, "epoch": 0, "global_step": 0}
    d = tmp_path_factory.mktemp("align_long")
    torch.save(ck, d / "ref_style.ckpt")
    pcm = (synth_wave(SECS) * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    wav = str(d / "rec.wav")
    with wavmod.open(wav, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000); f.writeframes(pcm.numpy().tobytes())
    tr = AsrTranslator(str(d / "ref_style.ckpt"), map_location="cuda")
    logp1, duration = tr.encode_long(wav, batch_size=1, **WIN)
    assert duration == SECS
    return tr, pcm, wav, logp1, d


def greedy_ids(logp, blank):
    am = torch.argmax(logp, dim=-1).tolist()
    return [c for i, c in enumerate(am) if c != blank and (i == 0 or am[i - 1] != c)]


def test_encode_long_is_the_streaming_rows(dev, setup):
    from lightning_asr_amd import streaming
    tr, pcm, wav, logp1, _ = setup
    rec = tr.stream(chunk_s=WIN["window_s"], left_s=WIN["context_s"], right_s=WIN["context_s"], max_segment_s=30.0,
                    endpoint_silence_s=None, dither=False, keep_logp=True)
    for i in range(0, pcm.numel(), 48000):
        rec.feed(pcm[i:i + 48000])
    fin = rec.finish()
    assert logp1.shape == (streaming.total_frames(pcm.numel()), 29) == (3001, 29) and logp1.dtype == torch.float32
    assert torch.equal(logp1, fin["logp"])
    plan = streaming.plan_windows(pcm.numel(), True, 128000, 32000, 32000, 0)
    lengths = [s1 - s0 for s0, s1, _, _ in plan]
    assert len(plan) == 8 and len(set(lengths)) == 3 and lengths.count(192000) == 6     # six equal windows, first and last of their own


def test_batched_windows_against_single(dev, setup):
    tr, pcm, wav, logp1, _ = setup
    logp4, _ = tr.encode_long(wav, batch_size=4, **WIN)
    assert logp4.shape == logp1.shape
    diff = float((logp4 - logp1).abs().max())
    print("encode_long batch_size=4 vs 1: max abs difference %.9g" % diff)
    top2 = torch.topk(logp1, 2, dim=-1).values
    sure = (top2[:, 0] - top2[:, 1]) > diff
    assert int(sure.sum()) > 0
    assert torch.equal(torch.argmax(logp4, -1)[sure], torch.argmax(logp1, -1)[sure])
    assert diff <= 2.0 * BATCH_DIFF_MEASURED, (diff, BATCH_DIFF_MEASURED)


def test_align_long_on_the_greedy_hypothesis(dev, setup):
    from lightning_asr_amd import ops
    tr, pcm, wav, logp1, _ = setup
    blank = len(tr.labels)
    ids = greedy_ids(logp1, blank)
    hyp = "".join(tr.labels[c] for c in ids)
    print("greedy hypothesis: %d labels on %d frames: %r" % (len(ids), logp1.shape[0], hyp[:80]))
    assert len(ids) >= 12
    al = ops.ctc_align_long(logp1.unsqueeze(0), torch.tensor([ids], device=dev), None, torch.tensor([len(ids)], dtype=torch.int32, device=dev),
                            blank, band=256)
    assert int(al.status[0]) == 0
    st = al.frame_state[0].tolist()
    assert A.valid_path(st, len(ids)) and A.collapse(st, ids, blank) == ids
    res = tr.align_long(wav, hyp, band=256, batch_size=1, **WIN)
    assert res["band"] == 256 and res["duration"] == SECS and res["score"] == float(al.score[0])
    words = res["words"]
    assert [w["word"] for w in words] == hyp.split()
    for w in words:
        assert 0.0 <= w["start"] < w["end"] <= SECS and 0.0 < w["score"] <= 1.0
    for a, b in zip(words, words[1:]):
        assert a["end"] <= b["start"]
    assert len(res["sentences"]) == 1 and res["sentences"][0]["text"] == hyp and res["sentences"][0]["n_words"] == len(words)
    if words:
        assert res["sentences"][0]["min_word_score"] == min(w["score"] for w in words)
    with pytest.raises(ValueError, match="too long"):
        tr.align_long(wav, "ab" * 2000, **WIN)                     # 4000 labels on 3001 frames


def test_cut_corpus_writes_a_trainable_manifest(dev, setup):
    from lightning_asr_amd.data_module import LibriDataModule, load_wav
    tr, pcm, wav, logp1, d = setup
    blank = len(tr.labels)
    chars = "".join(tr.labels[c] for c in greedy_ids(logp1, blank)).replace(" ", "")
    assert len(chars) >= 12
    piece = -(-len(chars) // 12)
    sentences = [chars[i:i + piece] for i in range(0, len(chars), piece)]     # about 5 s of the recording each
    out_dir, man = str(d / "cut"), str(d / "cut.json")
    res = tr.cut_corpus(wav, sentences, out_dir, man, max_duration=16.7, **WIN)
    lines = [json.loads(l) for l in open(man, encoding="utf-8") if l.strip()]
    assert lines == res["utterances"] and len(lines) >= 2 and res["dropped"] == []
    assert " ".join(l["text"] for l in lines) == " ".join(sentences)
    # every wav is its span of the recording sample for sample (PCM16 in, PCM16 out), and neighbours share their cut
    ref = pcm.to(torch.float32) / 32768.0
    spans = res["spans"]
    assert len(spans) == len(lines) and spans[0][0] >= 0 and spans[-1][1] <= pcm.numel()
    for l, (s0, s1) in zip(lines, spans):
        # (a score may underflow to 0 here: the formula weights' log-probs are in the 1e5s and the transcript forces spaces)
        assert set(l) == {"audio_filepath", "duration", "text", "score"} and 0.0 <= l["score"] <= 1.0
        assert l["duration"] == (s1 - s0) / 16000.0 and 0 < l["duration"] <= 16.7
        assert torch.equal(load_wav(l["audio_filepath"])[0], ref[s0:s1])
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    dm = LibriDataModule(man, man, man, tr.labels, train_bs=2, dev_bs=2, device="cuda")
    dm.setup()
    assert len(dm.train_datasets) == len(lines) == len(dm.dev_datasets)
    w0, ids0, path0 = dm.train_datasets[0]
    assert path0 == lines[0]["audio_filepath"] and ids0 == tr.text_to_ids(lines[0]["text"]) and w0.numel() == spans[0][1] - spans[0][0]
    # a second call appends; min_score above every score drops everything
    res2 = tr.cut_corpus(wav, sentences, out_dir, man, max_duration=16.7, min_score=2.0, **WIN)
    assert res2["utterances"] == [] and len(res2["dropped"]) == len(lines)
    assert len([l for l in open(man, encoding="utf-8") if l.strip()]) == len(lines)
