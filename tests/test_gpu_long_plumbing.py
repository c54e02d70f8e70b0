"""GPU tier of ``AsrTranslator.translate_long``: a recording is cut into utterances on the device (``ops.vad_segments``), gathered
into batch rows, decoded by translate()'s chain and timed relative to the recording.  The recording is the six-second hand case
of tests/helpers/vad_oracle.py (two segments: 0.4-2.1 s and 3.9-5.73 s), the checkpoint has formula weights."""
import os
import sys
import wave as wavmod

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vad_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

FRAME = 0.01                 # one segmenter frame in seconds


def _write_wav(path, rate, pcm):
    with wavmod.open(str(path), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(rate); f.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


def _checkpoint(tmp_path):
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
    return str(path)


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    """the files, the translator and ONE reference run of translate_long, shared by the tests below and left unchanged"""
    from lightning_asr_amd.predict import AsrTranslator
    d = tmp_path_factory.mktemp("long")
    pcm = O.recording_6s()
    _write_wav(d / "rec16.wav", 16000, pcm)
    _write_wav(d / "rec8.wav", 8000, O.recording_6s(rate=8000))
    _write_wav(d / "zero.wav", 16000, np.zeros(48000, dtype=np.int16))
    ckpt = _checkpoint(d)
    tr = AsrTranslator(ckpt, map_location="cuda")
    dith = tr.audio_parser.device_dither()
    step0 = dith.step.clone()
    res = tr.translate_long(str(d / "rec16.wav"))
    want, _, _ = O.segment(pcm, O.params())
    return {"dir": d, "pcm": pcm, "ckpt": ckpt, "tr": tr, "step0": step0, "res": res, "want": [tuple(s) for s in want.tolist()]}


def _bounds(res):
    return [(s["start"], s["end"]) for s in res["segments"]]


def test_segments_are_the_oracles(world):
    res = world["res"]
    assert world["want"] == [(6400, 33600), (62400, 91680)]
    assert res["duration"] == 6.0 and len(res["segments"]) == 2
    for (a, b), (s, e) in zip(_bounds(res), world["want"]):
        assert abs(a - s / 16000.0) < FRAME and abs(b - e / 16000.0) < FRAME
    assert _bounds(res) == [(0.4, 2.1), (3.9, 5.73)]                          # in time order, exact: every border is a frame border
    assert set(res) == {"text", "duration", "segments"} and all(set(s) == {"start", "end", "text", "words"} for s in res["segments"])


def test_texts_are_the_chain_spelled_out_by_hand(world, dev):
    from lightning_asr_amd import ops
    from lightning_asr_amd.data_module import load_wav
    tr, res = world["tr"], world["res"]
    dith = tr.audio_parser.device_dither()
    dith.step.copy_(world["step0"])
    wave = load_wav(str(world["dir"] / "rec16.wav"))[0].to(dev)
    assert torch.equal(wave, (torch.from_numpy(world["pcm"]).float() / 32768.0).to(dev))
    order = sorted(range(2), key=lambda i: world["want"][i][0] - world["want"][i][1])      # longest first: the second segment
    assert order == [1, 0]
    rows, lens = ops.gather_segments(wave, [(0,) + world["want"][i] for i in order])
    assert rows.shape == (2, 29280) and lens.tolist() == [29280, 27200]
    inputs, pct = tr.audio_parser.features_device(rows, lens, None, True, logical_len=rows.shape[1])
    out = tr.model._encode(inputs, pct)
    t_lens = ops.mask_lengths(pct, out.shape[1])
    tokens, n = ops.greedy_decode(tr.model.encoder.last_argmax.to(torch.int32).contiguous(), t_lens, len(tr.labels))
    texts = {}
    for j, i in enumerate(order):
        texts[i] = "".join(tr.labels[c] for c in tokens[j, :int(n[j])].tolist())
    assert [s["text"] for s in res["segments"]] == [texts[0], texts[1]]
    assert res["text"] == " ".join([texts[0], texts[1]])
    dith.step.copy_(world["step0"])
    again = tr.translate_long(str(world["dir"] / "rec16.wav"))
    assert again == res                                                       # the same dither step: the same result, times and scores included
    dith.step.copy_(world["step0"])
    untimed = tr.translate_long(str(world["dir"] / "rec16.wav"), timed=False)
    assert [s["words"] for s in untimed["segments"]] == [None, None] and untimed["text"] == res["text"]


def test_word_times_lie_inside_their_segment(world, dev):
    from lightning_asr_amd.data_module import load_wav
    tr, res = world["tr"], world["res"]
    for seg in res["segments"]:
        assert seg["words"] is not None and [w["word"] for w in seg["words"]] == seg["text"].split()
        for w in seg["words"]:
            assert seg["start"] <= w["start"] <= w["end"] <= seg["end"]
    # formula weights may decode to nothing, so a given transcript goes through the same batch path
    wave = load_wav(str(world["dir"] / "rec16.wav"))[0].to(dev)
    segs = [world["want"][1], world["want"][0]]
    out, t_lens = tr._segment_batch(wave, segs)
    ids = [tr.text_to_ids("hello world"), tr.text_to_ids("good day to you")]
    recs = tr._align_batch(out, t_lens, ids, segs)
    assert [[w["word"] for w in r] for r in recs] == [["hello", "world"], ["good", "day", "to", "you"]]
    for r, (s, e) in zip(recs, segs):
        times = [t for w in r for t in (w["start"], w["end"])]
        assert times == sorted(times) and s / 16000.0 <= times[0] and times[-1] <= e / 16000.0 and times[-1] > times[0]
        for w in r:
            assert all(w["start"] <= l["start"] < l["end"] <= w["end"] for l in w["labels"])
    assert tr._align_batch(out, t_lens, [[], tr.text_to_ids("a")], segs)[0] == []
    too_long = tr._align_batch(out, t_lens, [tr.text_to_ids("ab" * 800), tr.text_to_ids("a")], segs)
    assert too_long[0] is None and too_long[1] is not None


def test_a_silent_file_launches_no_forward(world, monkeypatch):
    tr = world["tr"]

    def boom(*a, **k):
        raise AssertionError("a forward was launched for a recording without speech")

    monkeypatch.setattr(tr.model, "_encode", boom)
    res = tr.translate_long(str(world["dir"] / "zero.wav"))
    assert res["text"] == "" and res["segments"] == [] and res["duration"] == 3.0


def test_batch_size_does_not_move_the_boundaries(world):
    tr = world["tr"]
    one = tr.translate_long(str(world["dir"] / "rec16.wav"), batch_size=1)
    many = tr.translate_long(str(world["dir"] / "rec16.wav"), batch_size=32)
    assert _bounds(one) == _bounds(many) == _bounds(world["res"])
    with pytest.raises(ValueError, match="batch_size"):
        tr.translate_long(str(world["dir"] / "rec16.wav"), batch_size=0)


def test_an_8k_copy_is_heard_at_its_true_times(world):
    tr = world["tr"]
    res = tr.translate_long(str(world["dir"] / "rec8.wav"), resample=True)
    assert res["duration"] == 6.0 and len(res["segments"]) == 2
    for (a, b), (s, e) in zip(_bounds(res), _bounds(world["res"])):
        assert abs(a - s) <= FRAME + 1e-9 and abs(b - e) <= FRAME + 1e-9
    raw = tr.translate_long(str(world["dir"] / "rec8.wav"))                   # without resample: 48000 samples taken for 16 kHz
    assert raw["duration"] == 3.0


def test_too_many_segments_is_an_error_that_names_the_parameter(world):
    with pytest.raises(ValueError, match="max_segments"):
        world["tr"].translate_long(str(world["dir"] / "rec16.wav"), max_segments=1)
    with pytest.raises(TypeError):
        world["tr"].translate_long(str(world["dir"] / "rec16.wav"), no_such_keyword=1)


def test_smaller_segments_through_the_vad_keywords(world):
    """max_segment_s reaches the segmenter: no segment is longer, together they still cover what the defaults found"""
    res = world["tr"].translate_long(str(world["dir"] / "rec16.wav"), batch_size=3, max_segment_s=0.5)
    b = _bounds(res)
    assert len(b) > 4 and all(e - s <= 0.5 + 1e-9 for s, e in b) and b == sorted(b)
    assert b[0][0] == 0.4 and b[-1][1] == 5.73 and sum(e - s for s, e in b) == pytest.approx(1.7 + 1.83)


def test_beam_decoder_runs_on_the_same_boundaries(world):
    from lightning_asr_amd.predict import AsrTranslator
    tr = AsrTranslator(world["ckpt"], map_location="cuda", decoder="beam", beam_width=4)
    res = tr.translate_long(str(world["dir"] / "rec16.wav"))
    assert _bounds(res) == _bounds(world["res"])
    for seg in res["segments"]:
        assert isinstance(seg["text"], str) and [w["word"] for w in seg["words"]] == seg["text"].split()


def test_a_segment_shorter_than_the_models_shortest_input(world):
    """a 0.1 s burst pads to a 0.3 s segment: 31 feature frames, fewer than the forward takes - its batch row is widened, its
    length and its times are its own"""
    from lightning_asr_amd.predict import MIN_ROW_SAMPLES
    rng = np.random.RandomState(3)
    y = 0.001 * rng.standard_normal(16000)
    y[6400:8000] += 0.3 * np.sin(2 * np.pi * 440.0 * np.arange(1600) / 16000.0)
    pcm = np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)
    want, _, _ = O.segment(pcm, O.params())
    assert want.tolist() == [[4800, 9600]] and 9600 - 4800 < MIN_ROW_SAMPLES
    _write_wav(world["dir"] / "short.wav", 16000, pcm)
    res = world["tr"].translate_long(str(world["dir"] / "short.wav"))
    assert _bounds(res) == [(0.3, 0.6)] and res["duration"] == 1.0
    for w in res["segments"][0]["words"]:
        assert 0.3 <= w["start"] <= w["end"] <= 0.6
