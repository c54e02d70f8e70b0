"""GPU tier of what is built on the resampler: any-rate files through ``AudioParser`` / ``AsrTranslator`` (resample=True), and speed
perturbation on every route that yields training batches (native ingest, the DataLoader collate, ``HostWaveSource``) and through
``Trainer.fit``.  With the options at their defaults the same tests pin today's results: the features of a 16 kHz file, the
half-length log-probs of an 8 kHz file, and the native batches (the files' own samples, lengths, pitch, key and rectangles)."""
import json
import math
import os
import random
import subprocess
import sys
import wave as wavmod
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import resample_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

LABELS = [c.strip() for c in open(os.path.join(ROOT, "data", "labels.txt")).readlines()]
FACTORS = [0.9, 1.0, 1.1]


def _write_wav(path, rate, pcm):
    with wavmod.open(str(path), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(rate); f.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


def _tone(n, rate, seed):
    g = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    y = 0.3 * np.sin(2 * math.pi * (220 + 180 * t) * t) + 0.05 * g.standard_normal(n)
    return (np.clip(y, -1, 1) * 32767).astype(np.int16)


def _bank_taps(rs, i):
    img = rs.bank.cpu().numpy()
    up, down, width, taps, offset = [int(v) for v in img[16 + 8 * i:21 + 8 * i]]
    return img.view(np.float32)[offset:offset + up * taps].reshape(taps, up).T.astype(np.float64)


# ------------------------------------------------------------------------------------------------ inference: any-rate audio in
def test_parse_audio_resamples_other_rates_and_leaves_16k_alone(dev, tmp_path):
    from lightning_asr_amd import ops
    from lightning_asr_amd.data_module import AudioParser, load_wav
    ap = AudioParser(device=str(dev))
    dith = ap.device_dither()
    p44 = tmp_path / "a44.wav"
    _write_wav(p44, 44100, _tone(13230, 44100, 1))                    # 0.3 s
    step0 = dith.step.clone()
    got = ap.parse_audio(str(p44), mask=False, resample=True)
    dith.step.copy_(step0)
    wave = load_wav(str(p44))[0].to(dev)
    y16, n16 = ops.resample(wave, 44100, 16000)
    assert int(n16[0]) == y16.numel() == 4800
    want = ap.features([y16], False)[0]
    assert got.shape == want.shape == (1, 1, 64, 1 + (4800 + 64) // 160) and torch.equal(got, want)
    dith.step.copy_(step0)
    raw = ap.parse_audio(str(p44), mask=False)                        # the default: the samples as they are, 13230 of them
    assert raw.shape[-1] == 1 + (13230 + 64) // 160
    p16 = tmp_path / "a16.wav"
    _write_wav(p16, 16000, _tone(4800, 16000, 2))
    dith.step.copy_(step0)
    a = ap.parse_audio(str(p16), mask=False, resample=True)
    dith.step.copy_(step0)
    b = ap.parse_audio(str(p16), mask=False, resample=False)
    dith.step.copy_(step0)
    c = ap.features([load_wav(str(p16))[0]], False, leads=[0])[0]     # today's chain, spelled out
    assert torch.equal(a, b) and torch.equal(b, c)


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


def test_translator_hears_an_8k_file_at_its_true_speed(dev, tmp_path):
    from lightning_asr_amd.data_module import load_wav
    from lightning_asr_amd.predict import AsrTranslator
    ckpt = _checkpoint(tmp_path)
    p8 = tmp_path / "a8.wav"
    _write_wav(p8, 8000, _tone(8000, 8000, 3))                        # 1 s
    tr = AsrTranslator(ckpt, map_location="cuda", resample=True)
    frame = tr.frame_seconds()
    dith = tr.audio_parser.device_dither()
    step0 = dith.step.clone()
    out_t, dur_t = tr._encode_file(str(p8))
    assert dur_t == 1.0 and out_t.shape[1] == tr.model.encoder.native.out_frames(1 + (16000 + 64) // 160)
    dith.step.copy_(step0)
    text, words = tr.translate_timed(str(p8))
    dith.step.copy_(step0)
    assert text == tr.translate(str(p8)) and [w["word"] for w in words] == text.split()
    if words:      # formula weights may decode to nothing: then the align() below, whose transcript is given, carries the time-scale check
        assert words[-1]["end"] <= 1.0 + frame
    dith.step.copy_(step0)
    al = tr.align(str(p8), "hello world")
    assert [w["word"] for w in al] == ["hello", "world"] and al[-1]["end"] <= 1.0 + frame
    assert tr.translate_nbest(str(p8), 2)
    # resample=False - per call or as the translator's default - is today's result: 8000 samples taken for 16 kHz
    tr0 = AsrTranslator(ckpt, map_location="cuda")
    assert tr0.resample is False
    d0 = tr0.audio_parser.device_dither()
    s0 = d0.step.clone()
    out_f, dur_f = tr0._encode_file(str(p8))
    d0.step.copy_(s0)
    inputs = tr0.audio_parser.features([load_wav(str(p8))[0]], False, leads=[0])[0]
    today = tr0.model._encode(inputs, torch.ones(1, device=dev))
    assert dur_f == 0.5 and out_f.shape[1] == tr0.model.encoder.native.out_frames(1 + (8000 + 64) // 160) and torch.equal(out_f, today)
    out_o, dur_o = tr._encode_file(str(p8), resample=False)           # the per-call override of a resampling translator
    assert dur_o == 0.5 and out_o.shape == out_f.shape
    al0 = tr0.align(str(p8), "hello")
    assert al0[-1]["end"] <= 0.5 + frame
    # the manifest loaders do not resample: with resample=True a file of another rate is refused by name, not mis-decoded
    p16 = tmp_path / "a16.wav"
    _write_wav(p16, 16000, _tone(16000, 16000, 4))
    man = tmp_path / "m.json"
    with open(man, "w") as f:
        f.write(json.dumps({"audio_filepath": str(p16), "duration": 1.0, "text": "a b"}) + "\n")
        f.write(json.dumps({"audio_filepath": str(p8), "duration": 1.0, "text": "a b"}) + "\n")
    with pytest.raises(ValueError, match="a8.wav"):
        tr.evalute_manifest(str(man), batch_size=2)
    with pytest.raises(ValueError, match="a8.wav"):
        tr.align_manifest(str(man), str(tmp_path / "al.jsonl"), batch_size=2)
    assert len(tr0.align_manifest(str(man), str(tmp_path / "al0.jsonl"), batch_size=2)) == 2       # the default still takes it as it is


# ------------------------------------------------------------------------------------------------ training: speed perturbation
def _six_wavs(tmp_path):
    from lightning_asr_amd.data_module import MyAudioDataset
    man = tmp_path / "m.json"
    pcms = []
    with open(man, "w") as f:
        for i in range(6):
            n = 3000 + 517 * i
            pcm = _tone(n, 16000, 10 + i)
            pcms.append(pcm)
            p = tmp_path / ("c%d.wav" % i)
            _write_wav(p, 16000, pcm)
            f.write(json.dumps({"audio_filepath": str(p), "duration": n / 16000.0, "text": "abc"[: 1 + i % 3] + "g"}) + "\n")
    return MyAudioDataset([str(man)], list("abcdefg"), mask=True), pcms


def _run_native(dev, ds, seed, speed_perturb):
    from lightning_asr_amd.data_module import AudioParser
    from lightning_asr_amd.fused_fit import NativeSource
    ap = AudioParser(device=str(dev))
    ap.rand = random.Random(seed)
    src = NativeSource(ds, [[0, 1, 2], [3, 4, 5]], ap, dev, batch_size=3, max_seconds=1.0, mask=True, n_threads=2, limit=2, crop=False,
                       speed_perturb=speed_perturb)
    got = []
    try:
        for db in src:
            torch.cuda.current_stream().wait_event(db.ready)
            got.append({"pcm": db.pcm.clone(), "lens": db.lens.clone(), "aug": db.aug.clone(), "targets": db.targets.clone(),
                        "sizes": db.sizes.clone(), "L": db.L, "pitch": db.pitch, "key": db.key, "seconds": db.seconds, "speed": db.speed,
                        "B": db.B, "S": db.S, "ld": db.ld})
            src.release(db)
    finally:
        src.close()
    torch.cuda.synchronize()
    return got, ap


def test_native_source_applies_speed_perturbation(dev, tmp_path):
    from lightning_asr_amd.data_module import AudioParser, parse_speed_factors
    ds, pcms = _six_wavs(tmp_path)
    got, ap = _run_native(dev, ds, 5, FACTORS)
    assert len(got) == 2
    # the draws, replayed: per utterance its factor, then its SpecAugment rectangle for the RESAMPLED length
    twin = AudioParser.__new__(AudioParser)
    twin.rand = random.Random(5)
    twin.speed_factors = parse_speed_factors(FACTORS)
    rs = ap.speed_resampler()
    assert rs.factors == [(10, 9), (1, 1), (10, 11)]
    seen_factors = set()
    for bi, b in enumerate(got):
        ks, rects, n_out = [], [], []
        for i in range(3):
            n = pcms[3 * bi + i].size
            ks.append(twin.draw_speed())
            f = twin.speed_factors[ks[-1]]
            n_out.append(int(math.ceil(Fraction(n) / f)))
            rects.append(twin.draw_spec_augment(1 + (n_out[-1] + 64) // 160))
        seen_factors.update(ks)
        assert b["speed"] == ks and b["aug"].cpu().tolist() == [list(r) for r in rects]
        assert b["lens"].cpu().tolist() == n_out
        frames = 1 + (max(n_out) + 64) // 160
        assert b["L"] == 160 * (frames - 1) + 95 and b["pitch"] == b["L"] + 1 and b["pcm"].shape == (3, b["pitch"])
        assert b["key"] == (3, b["pitch"], b["L"], b["S"], True) and b["pcm"].dtype == torch.int16
        assert abs(b["seconds"] - sum(n_out) / 16000.0) < 1e-9
        rows = b["pcm"].cpu().numpy()
        for i in range(3):
            pcm, k = pcms[3 * bi + i], ks[i]
            assert not rows[i, n_out[i]:].any()
            if twin.speed_factors[k] == 1:
                assert np.array_equal(rows[i, :n_out[i]], pcm)                                   # factor 1.0: the file, bit for bit
                continue
            f = twin.speed_factors[k]
            y, a = O.resample(pcm.astype(np.float64) / 32768.0, f.numerator, f.denominator, h=_bank_taps(rs, k))
            taps = O.geometry(f.numerator, f.denominator)[3]
            err = np.abs(rows[i, :n_out[i]].astype(np.float64) - np.clip(32768.0 * y, -32768, 32767))
            assert y.size == n_out[i] and (err <= 0.5 + 32768.0 * (taps + 1) * 2.0 ** -24 * a).all()
    assert len(seen_factors) >= 2                                                                 # (seed 5 does draw different factors)


def test_native_source_without_the_key_is_todays_batches(dev, tmp_path):
    """speed_perturb absent and [] give the same batches, and those are what the route has always produced for crop=False: the
    files' own samples and lengths, one pitch per frame-count class, rectangles drawn for the file lengths in file order"""
    from lightning_asr_amd.data_module import AudioParser
    ds, pcms = _six_wavs(tmp_path)
    a, _ = _run_native(dev, ds, 5, None)
    b, _ = _run_native(dev, ds, 5, [])
    twin = AudioParser.__new__(AudioParser)
    twin.rand = random.Random(5)
    for bi, (x, y) in enumerate(zip(a, b)):
        # An unperturbed row is written up to the host reader's pitch `ld`: the file's samples, then zeros.  Past it the class-pitch
        # row is never written nor read (DeviceFeeder.upload) and holds whatever the slot's block held before: not compared.
        ld = x["ld"]
        assert ld == y["ld"] and ld <= x["pitch"] == y["pitch"]
        for k in x:
            u, v = (x[k][:, :ld], y[k][:, :ld]) if k == "pcm" else (x[k], y[k])
            same = torch.equal(u, v) if isinstance(u, torch.Tensor) else u == v
            assert same, k
        ns = [pcms[3 * bi + i].size for i in range(3)]
        assert x["speed"] is None and x["lens"].cpu().tolist() == ns
        assert x["aug"].cpu().tolist() == [list(twin.draw_spec_augment(1 + (n + 64) // 160)) for n in ns]
        frames = 1 + (max(ns) + 64) // 160
        assert x["L"] == 160 * (frames - 1) + 95 and x["pitch"] == x["L"] + 1 and x["key"] == (3, x["pitch"], x["L"], x["S"], True)
        rows = x["pcm"].cpu().numpy()
        for i in range(3):
            assert np.array_equal(rows[i, :ns[i]], pcms[3 * bi + i]) and not rows[i, ns[i]:ld].any()


def test_loader_routes_apply_speed_perturbation(dev, tmp_path):
    """the DataLoader collate (-> on_after_batch_transfer) and HostWaveSource resample through the parser's ops.Resampler"""
    from lightning_asr_amd.data_module import LibriDataModule, load_wav
    from lightning_asr_amd.fused_fit import HostWaveSource
    ds, pcms = _six_wavs(tmp_path)
    man = str(tmp_path / "m.json")
    dm = LibriDataModule([man], man, man, list("abcdefg"), train_bs=3, dev_bs=3, num_worker=0, device=str(dev), train_crop=False,
                         speed_perturb=FACTORS)
    dm.setup()
    ap = dm.audio_parser
    items = [dm.train_datasets[i] for i in range(3)]
    wb = dm._collate_train(items)
    assert wb.leads is None
    assert dm.draw_speed_batch(3, False) is None                       # evaluation batches are never perturbed
    dith = ap.device_dither()
    step0 = dith.step.clone()
    ap.rand = random.Random(21)                                        # the factors are drawn in the main process, then the rectangles
    inputs, _, pct, _, _ = dm.on_after_batch_transfer(wb)
    rs = ap.speed_resampler()
    ap.rand = random.Random(21)
    speed = dm.draw_speed_batch(3, True)
    assert len(speed) == 3
    singles = []
    for w, k in zip(wb[0], speed):
        out, n = rs(w.to(dev).unsqueeze(0), conv_id=torch.tensor([k], dtype=torch.int32, device=dev))
        singles.append(out[0, :int(n[0])])
        assert int(n[0]) == ap.speed_out_len(w.numel(), k)
    dith.step.copy_(step0)
    want, want_pct = ap.features(singles, True)                        # (its rectangles continue the stream the factors came from)
    assert torch.equal(inputs, want) and torch.equal(pct, want_pct)
    # HostWaveSource over the same loader
    ap.rand = random.Random(9)
    src = HostWaveSource(dm.train_dataloader(), dev, 2, audio_parser=ap)
    n_seen = 0
    for db in src:
        assert db.speed is not None and db.pcm.dtype == torch.float32
        files = {p: load_wav(p)[0] for p in db.paths}
        for i, p in enumerate(db.paths):
            n = ap.speed_out_len(files[p].numel(), db.speed[i])
            assert int(db.lens[i]) == n and not db.pcm[i, n:].any()
            one, _ = rs(files[p].to(dev).unsqueeze(0), conv_id=torch.tensor([db.speed[i]], dtype=torch.int32, device=dev))
            assert torch.equal(db.pcm[i, :n], one[0, :n])
        assert db.L == int(db.lens.max()) and db.pcm.shape[1] == db.pitch
        n_seen += 1
    assert n_seen == 2
    for bad in ([0.3], ["x"], [1.234567]):
        with pytest.raises(ValueError):
            LibriDataModule([man], man, man, list("abcdefg"), device=str(dev), speed_perturb=bad)
    dm2 = LibriDataModule([man], man, man, list("abcdefg"), device=str(dev))
    dm2.speed_perturb = [3.0]
    with pytest.raises(ValueError):
        dm2.setup()


def test_trainer_fit_with_speed_perturbation(dev, tmp_path):
    from lightning_asr_amd.data_module import LibriDataModule
    from lightning_asr_amd.lightning_compat import Trainer, seed_everything
    from lightning_asr_amd.train import LightingModule
    data = tmp_path / "synth"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_data.py"), "--out", str(data), "--n-train", "12", "--n-dev", "4",
                    "--seconds", "2.0"], check=True)
    seed_everything(0)
    dm = LibriDataModule([str(data / "train.json")], str(data / "dev.json"), str(data / "dev.json"), LABELS, train_bs=4, dev_bs=4,
                         num_worker=2, device=str(dev), act_dtype=torch.bfloat16, speed_perturb=FACTORS)
    model = LightingModule(learning_rate=1e-2, weight_decay=1e-3, labels=LABELS, total_epoch=1, drop_rate=0.0, mask=True, use_cer=True,
                           dtype="bf16", device=str(dev), warmup_steps=2)
    seen = []
    tr = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "run"), device=str(dev), check_val_every_n_epoch=1, log_every_n_steps=1)
    tr._fused_on_batch = lambda db: seen.append((db.speed, db.lens.clone(), db.pitch, db.L))
    hist = tr.fit(model, dm)
    assert tr.fused is not None and tr.fused.source_kind == "NativeSource" and tr.global_step == 3 and len(seen) == 3
    assert np.isfinite(hist[-1]["train_loss"]) and hist[-1]["train_loss"] > 0
    for speed, lens, pitch, L in seen:
        assert speed is not None and len(speed) == 4 and int(lens.max()) <= L < pitch
        assert all(int(n) < (1 << 30) for n in lens.tolist())           # no lead-in flags under speed perturbation
    assert len(set(k for s in seen for k in s[0])) >= 2
