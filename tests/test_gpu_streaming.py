"""AsrTranslator.stream / streaming.StreamingRecognizer on the GPU, with a small random-weight checkpoint and dither off:
packet-size invariance of the emitted log-prob rows and of the final record, the one-window case against the one-shot chain, the
multi-window rows against a loop written here from plan_windows, the text against the one-shot decode of the kept rows, a forced
max_segment_s commit, and the endpoint commit on trailing silence."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

CFG = dict(chunk_s=0.5, left_s=1.0, right_s=0.5, dither=False, keep_logp=True)
W = 4


def synth_wave(secs, seed=5):
    g = torch.Generator().manual_seed(seed)
    n = int(16000 * secs)
    t = torch.arange(n) / 16000.0
    y = 0.3 * torch.sin(2 * math.pi * (220 + 180 * t) * t) * (0.5 + 0.5 * torch.sin(2 * math.pi * 3.0 * t)) \
        + 0.05 * torch.randn(n, generator=g)
    return y.clamp(-1, 1).contiguous()


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """a reference-style checkpoint of formula weights, as tests/test_gpu_ctc_beam.py's translator tests build theirs"""
    from oracle import ref_cpu as R
    from lightning_asr_amd.predict import EN_LABELS
    state = R.formula_state("plain", 29)
    for k_ in state:
        if k_.endswith("running_var"):
            state[k_] = state[k_] * 0 + 0.5 + 0.01 * torch.arange(state[k_].numel()).float() % 1.0
    ck = {"state_dict": {"encoder." + k_: v for k_, v in state.items()},
          "hyper_parameters": {"learning_rate": 1e-2, "weight_decay": 1e-3, "labels": EN_LABELS, "total_epoch": 1, "drop_rate": 0.0,
                               "mask": True, "use_cer": False}, "epoch": 0, "global_step": 0}
    path = tmp_path_factory.mktemp("stream_ckpt") / "ref_style.ckpt"
    torch.save(ck, path)
    return str(path)


@pytest.fixture(scope="module")
def beam_tr(dev, ckpt):
    from lightning_asr_amd.predict import AsrTranslator
    return AsrTranslator(ckpt, map_location="cuda", decoder="beam", beam_width=W, cutoff_top_n=40)


@pytest.fixture(scope="module")
def greedy_tr(dev, ckpt):
    from lightning_asr_amd.predict import AsrTranslator
    return AsrTranslator(ckpt, map_location="cuda")


@pytest.fixture(scope="module")
def wave3():
    return synth_wave(3.0)


def stream_all(tr, wave, packet, **cfg):
    rec = tr.stream(**cfg)
    outs = []
    for i in range(0, wave.numel(), packet or wave.numel()):
        outs.append(rec.feed(wave[i:i + (packet or wave.numel())]))
    fin = rec.finish()
    return outs, fin


def one_shot_logp(tr, wave_dev):
    """translate()'s chain on the whole wave, dither off: log-probs (T', C) f32"""
    lens = torch.full((1,), wave_dev.numel(), dtype=torch.int32, device=wave_dev.device)
    with torch.no_grad():
        inputs, pct = tr.audio_parser.features_device(wave_dev[None].contiguous(), lens, None, False, logical_len=wave_dev.numel())
        return tr.model._encode(inputs, pct)[0].float()


def decode_rows(tr, rows) -> str:
    """the translator's own one-shot decoder on log-prob rows (T', C)"""
    if tr.decoder == "beam":
        return tr.beam(rows[None].contiguous(), None)[0]
    return tr.wer.ctc_decoder_predictions_tensor(torch.argmax(rows[None], dim=-1))[0]


def test_packet_size_does_not_change_rows_or_record(dev, beam_tr, wave3):
    runs = {p: stream_all(beam_tr, wave3, p, **CFG) for p in (1600, 7777, None)}
    _, ref = runs[None]
    assert ref["final"] is True and ref["frames"] == ref["logp"].shape[0] == ((wave3.numel() + 64) // 160) // 2 + 1
    for p, (outs, fin) in runs.items():
        assert torch.equal(fin["logp"], ref["logp"]), p
        assert {k: v for k, v in fin.items() if k != "logp"} == {k: v for k, v in ref.items() if k != "logp"}, p
        assert all(o["final"] is False and o["text"] == " ".join(t for t in (o["committed"], o["partial"]) if t) for o in outs)
        assert [o["frames"] for o in outs] == sorted(o["frames"] for o in outs)
    # int16 PCM and a device tensor are the same audio
    pcm = (wave3 * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    _, a = stream_all(beam_tr, pcm, 4000, **CFG)
    _, b = stream_all(beam_tr, (pcm.to(torch.float32) / 32768.0).to(dev), 4000, **CFG)
    assert torch.equal(a["logp"], b["logp"]) and a["text"] == b["text"]


@pytest.mark.parametrize("which", ["greedy", "beam"])
def test_one_window_is_the_one_shot_chain(dev, beam_tr, greedy_tr, wave3, which):
    tr = beam_tr if which == "beam" else greedy_tr
    _, fin = stream_all(tr, wave3, 7777, chunk_s=4.0, left_s=1.0, right_s=0.5, dither=False, keep_logp=True,
                        endpoint_silence_s=None)
    want = one_shot_logp(tr, wave3.to(dev))
    assert torch.equal(fin["logp"], want)
    assert fin["text"] == decode_rows(tr, want)
    assert fin["frames"] == want.shape[0]


def test_rows_equal_a_loop_over_the_plan(dev, beam_tr, wave3):
    from lightning_asr_amd.predict import MIN_ROW_SAMPLES
    from lightning_asr_amd.streaming import plan_windows
    tr = beam_tr
    _, fin = stream_all(tr, wave3, 1600, endpoint_silence_s=None, **CFG)
    native = tr.model.encoder.native
    wave = wave3.to(dev)
    rows = []
    plan = plan_windows(wave.numel(), True, 8000, 16000, 8000, 0, native.out_frames)
    assert len(plan) >= 4
    for s0, s1, first, n in plan:
        row = torch.zeros(1, max(s1 - s0, MIN_ROW_SAMPLES), device=dev)
        row[0, :s1 - s0] = wave[s0:s1]
        lens = torch.full((1,), s1 - s0, dtype=torch.int32, device=dev)
        with torch.no_grad():
            inputs, pct = tr.audio_parser.features_device(row, lens, None, False, logical_len=row.shape[1])
            rows.append(tr.model._encode(inputs, pct)[0, first:first + n].float())
    want = torch.cat(rows)
    assert torch.equal(fin["logp"], want)
    # and the text is the one-shot beam decode of those rows
    assert fin["text"] == decode_rows(tr, want)
    assert fin["committed"] == fin["text"] and fin["partial"] == ""


def test_max_segment_forces_a_commit(dev, beam_tr, wave3):
    from lightning_asr_amd.streaming import join_texts
    tr = beam_tr
    outs, fin = stream_all(tr, wave3, 1600, max_segment_s=2.0, endpoint_silence_s=None, **CFG)
    rows = fin["logp"]
    assert rows.shape[0] == 151
    parts = [decode_rows(tr, rows[:100]), decode_rows(tr, rows[100:])]
    assert [(s["start_frame"], s["end_frame"]) for s in fin["segments"]] == [(0, 100), (100, 151)]
    assert [s["text"] for s in fin["segments"]] == parts
    assert fin["text"] == join_texts(parts, tr.labels)
    # before the 100th frame nothing is committed; after it the first segment's text is, unchanged to the end
    assert all(o["committed"] == "" for o in outs if o["frames"] < 100)
    assert all(o["committed"] == parts[0] for o in outs if o["frames"] >= 100)


def test_trailing_silence_commits_at_the_endpoint(dev, beam_tr):
    """A wave of 2 s of signal and 3 s of zeros, through the recogniser's own packets, buffer, windows and decoder.  The formula
    weights do not tell silence from signal (measured: the argmax of every emitted frame of this wave is class 15, zeros or
    not), and no trained checkpoint ships with the project, so the acoustic model alone is stood in for: the rows a window
    emits are taken from a fixed (frames, C) table, labels over the signal and the blank over the zeros, cut by the window's own
    (s0, first, n).  Everything the endpoint rule itself consists of runs as shipped."""
    tr = beam_tr
    blank = len(tr.labels)
    wave = torch.cat([synth_wave(2.0, seed=6), torch.zeros(int(16000 * 3.0))])
    n_frames = ((wave.numel() + 64) // 160) // 2 + 1
    table = torch.full((n_frames, blank + 1), -12.0)
    for f in range(n_frames):
        label = 2 + (f // 6) % 5 if f < 100 and (f // 3) % 2 == 0 else blank       # 2 s of signal = 100 frames
        table[f, label] = 0.0
    table = torch.log_softmax(table, -1).to(dev)
    rec = tr.stream(endpoint_silence_s=0.8, **CFG)
    rec._window_logp = lambda s0, s1, first, n: table[s0 // 320 + first:s0 // 320 + first + n].contiguous()
    outs = [rec.feed(wave[i:i + 1600]) for i in range(0, wave.numel(), 1600)]
    assert torch.equal(rec.logp, table[:rec.frames])
    assert any(o["committed"] for o in outs), "no endpoint commit before finish()"
    first = next(o for o in outs if o["committed"])
    assert first["partial"] == "" and first["text"] == first["committed"]
    # the commit came at the end of the first step whose last 40 frames are all blank (0.8 s; steps are 25 frames: frame 150),
    # and holds the one-shot decode of the frames up to there
    assert first["frames"] == 150
    assert all(o["partial"] for o in outs if 25 <= o["frames"] < 150)
    assert first["committed"] == decode_rows(tr, table[:150]) != ""
    # silence after the commit neither commits again nor adds text
    fin = rec.finish()
    assert fin["text"] == first["committed"] and len(fin["segments"]) == 2 and fin["segments"][1]["text"] == ""
    assert fin["frames"] == n_frames
