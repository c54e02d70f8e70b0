"""GPU tier of what is built on the noise and reverberation kernels: every route that yields training batches (native ingest, the
DataLoader collate, ``HostWaveSource``) applies them directly after the resampler, with the recorded draws, and leaves lengths,
pitch and graph key alone; ``Trainer.fit`` runs with every augmentation on; with the keys absent the batches and the calls into
the library are today's.

The rows are compared with the f64 oracle (tests/helpers/wave_aug_oracle.py) on the same inputs and draws.  Bound per sample, with
e_j = (K + 1) 2^-24 A_j the FIR's worst case:  g_s e_j  +  2^-22 (|g_s y_j| + |g_n v_j|)  for the mix, as in test_gpu_wave_aug.py,
plus - the gains here are the ORACLE's, not the kernel's - the kernel's own g_s and g_n moving with its E_y: |dE_y| <= 2 |e| sqrt(E_y)
gives a relative |e| / sqrt(E_y) on g_s (first order; 1 % is added for the second), and 1e-9 for the f64 energies.  PCM16 rows add
0.5 and scale by 32768 against the reference clamped as the operator clamps."""
import json
import math
import os
import random
import subprocess
import sys
import wave as wavmod

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import wave_aug_oracle as O  # noqa: E402

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


def _banks():
    rng = np.random.RandomState(8)
    rirs = []
    for K, d in ((200, 0), (1700, 30), (64, 63)):
        h = rng.standard_normal(K) * np.exp(-np.arange(K) / (K / 7.0))
        h[d] = 2.0 * np.abs(h).max() + 1.0
        rirs.append((h / h[d] * 0.5).astype(np.float32))
    noises = [np.rint(rng.uniform(-0.3, 0.3, n) * 32768).astype(np.int16) for n in (900, 7001)]
    return rirs, noises


def _wave_aug(dev, rir_prob=0.6, noise_prob=0.7):
    from lightning_asr_amd.data_module import WaveAug
    rirs, noises = _banks()
    return WaveAug(rirs, noises, rir_prob=rir_prob, noise_prob=noise_prob, noise_snr_db=(5, 20), device=str(dev))


def _check_row(got, x, word, wa, pcm16_out):
    """got: the row a route produced; x (n,) f64 its input; word = (rir_id, noise_id, start, snr_cdb)"""
    rir, nid, start, snr = word
    op = wa.op()
    h = d = None
    if rir >= 0:
        K, d = op.rir_taps[rir], op.rir_delay[rir]
        h = wa.rirs[rir][:K].astype(np.float64)
    clip = None
    if nid >= 0:                                             # the bank holds PCM16: f32 clips are rounded on the way in
        c = wa.noises[nid]
        clip = (c.astype(np.float64) if c.dtype == np.int16 else np.clip(np.rint(c.astype(np.float64) * 32768.0), -32768, 32767)) / 32768.0
    ref = O.augment(x, h, d or 0, clip, start, snr)
    gs, gn = ref["gains"]
    e = (len(h) + 1) * 2.0 ** -24 * ref["A"] if h is not None else np.zeros(x.size)
    rel = 1.01 * np.linalg.norm(e) / math.sqrt(ref["stats"][1]) + 1e-9 if ref["stats"][1] > 0 else 0.0
    mag = np.abs(gs * ref["y"]) + np.abs(gn * ref["v"])
    bound = gs * e + (2.0 ** -22 + rel) * mag
    want = ref["out"]
    if pcm16_out:
        want, bound = np.clip(32768.0 * want, -32768.0, 32767.0), 0.5 + 32768.0 * bound
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    assert (err <= bound).all(), (word, float((err / bound).max()))


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


def _run_native(dev, ds, seed, speed_perturb, wave_aug, mask=True):
    from lightning_asr_amd.data_module import AudioParser
    from lightning_asr_amd.fused_fit import NativeSource
    ap = AudioParser(device=str(dev))
    ap.rand = random.Random(seed)
    ap.wave_aug = wave_aug
    src = NativeSource(ds, [[0, 1, 2], [3, 4, 5]], ap, dev, batch_size=3, max_seconds=1.0, mask=mask, n_threads=2, limit=2, crop=False,
                       speed_perturb=speed_perturb)
    got = []
    try:
        for db in src:
            torch.cuda.current_stream().wait_event(db.ready)
            got.append({"pcm": db.pcm.clone(), "lens": db.lens.clone(), "aug": db.aug.clone() if db.aug is not None else None,
                        "targets": db.targets.clone(), "sizes": db.sizes.clone(), "L": db.L, "pitch": db.pitch, "key": db.key,
                        "seconds": db.seconds, "speed": db.speed, "wave_aug": db.wave_aug, "B": db.B, "S": db.S})
            src.release(db)
    finally:
        src.close()
    torch.cuda.synchronize()
    return got, ap


@pytest.mark.parametrize("speed", [False, True])
def test_native_source_applies_noise_and_reverb(dev, tmp_path, speed):
    from lightning_asr_amd.data_module import AudioParser, parse_speed_factors
    ds, pcms = _six_wavs(tmp_path)
    wa = _wave_aug(dev)
    got, ap = _run_native(dev, ds, 5, FACTORS if speed else [], wa)
    assert len(got) == 2
    twin = AudioParser.__new__(AudioParser)                 # the draws, replayed: speed factor, parameter word, rectangle per utterance
    twin.rand = random.Random(5)
    twin.speed_factors = parse_speed_factors(FACTORS if speed else [])
    twin.wave_aug = _wave_aug(dev)
    kinds = set()
    for bi, b in enumerate(got):
        ks, words, rects, n_out = [], [], [], []
        for i in range(3):
            n = pcms[3 * bi + i].size
            if speed:
                ks.append(twin.draw_speed())
                n = twin.speed_out_len(n, ks[-1])
            n_out.append(n)
            words.append(twin.draw_wave_aug())
            rects.append(list(twin.draw_spec_augment(1 + (n + 64) // 160)))
        assert b["wave_aug"] == words and b["speed"] == (ks if speed else None) and b["aug"].cpu().tolist() == rects
        assert b["lens"].cpu().tolist() == n_out, "the lengths do not change"
        frames = 1 + (max(n_out) + 64) // 160
        assert b["L"] == 160 * (frames - 1) + 95 and b["pitch"] == b["L"] + 1 and b["pcm"].shape == (3, b["pitch"])
        assert b["key"] == (3, b["pitch"], b["L"], b["S"], True) and b["pcm"].dtype == torch.int16
        rows = b["pcm"].cpu().numpy()
        for i in range(3):
            x = pcms[3 * bi + i]
            if speed:                                       # the resampled PCM16 row the augmentation saw: the same operator on the file
                xin = torch.from_numpy(x).to(dev).unsqueeze(0)
                out, n = ap.speed_resampler()(xin, conv_id=torch.tensor([ks[i]], dtype=torch.int32, device=dev))
                x = out[0, :int(n[0])].cpu().numpy()
            assert x.size == n_out[i] and not rows[i, n_out[i]:].any()
            kinds.add((words[i][0] >= 0, words[i][1] >= 0))
            if words[i][0] < 0 and words[i][1] < 0:
                assert np.array_equal(rows[i, :x.size], x)                                      # neither: the row, bit for bit
            else:
                _check_row(rows[i, :x.size], x.astype(np.float64) / 32768.0, words[i], wa, True)
    assert len(kinds) >= 3, kinds                            # (seed 5 does draw different kinds)


def test_without_the_keys_batches_and_library_calls_are_todays(dev, tmp_path, monkeypatch):
    """no WaveAug on the parser: the files' own samples and lengths, rectangles drawn for the file lengths in file order, and the
    only entry point of the library the route calls is the wav reader; an evaluation source never augments"""
    from lightning_asr_amd import _lib, ops
    from lightning_asr_amd.data_module import AudioParser
    ds, pcms = _six_wavs(tmp_path)
    calls = []
    real = _lib.call

    def recording(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recording)
    monkeypatch.setattr(ops, "call", recording)
    a, _ = _run_native(dev, ds, 5, None, None)
    assert set(calls) == {"lasr_wav_read_batch"} and len(calls) >= 2
    twin = AudioParser.__new__(AudioParser)
    twin.rand = random.Random(5)
    for bi, x in enumerate(a):
        ns = [pcms[3 * bi + i].size for i in range(3)]
        assert x["speed"] is None and x["wave_aug"] is None and x["lens"].cpu().tolist() == ns
        assert x["aug"].cpu().tolist() == [list(twin.draw_spec_augment(1 + (n + 64) // 160)) for n in ns]
        frames = 1 + (max(ns) + 64) // 160
        assert x["L"] == 160 * (frames - 1) + 95 and x["pitch"] == x["L"] + 1 and x["key"] == (3, x["pitch"], x["L"], x["S"], True)
        rows = x["pcm"].cpu().numpy()
        for i in range(3):
            assert np.array_equal(rows[i, :ns[i]], pcms[3 * bi + i])
    del calls[:]
    e, _ = _run_native(dev, ds, 5, None, _wave_aug(dev, 1.0, 1.0), mask=False)       # evaluation: the keys are set, nothing is applied
    assert set(calls) == {"lasr_wav_read_batch"}
    for bi, x in enumerate(e):
        assert x["wave_aug"] is None
        for i in range(3):
            assert np.array_equal(x["pcm"].cpu().numpy()[i, :pcms[3 * bi + i].size], pcms[3 * bi + i])


def _noise_and_rir_manifests(tmp_path):
    rirs, noises = _banks()
    out = {}
    for key, arrs, rate in (("noise", noises, 16000), ("rir", rirs, 16000)):
        man = tmp_path / (key + ".json")
        with open(man, "w") as f:
            for i, a in enumerate(arrs):
                p = tmp_path / ("%s%d.wav" % (key, i))
                _write_wav(p, rate, a if a.dtype == np.int16 else np.rint(a * 32767).astype(np.int16))
                f.write(json.dumps({"audio_filepath": str(p)}) + "\n")
        out[key] = str(man)
    return out


def test_loader_routes_apply_noise_and_reverb(dev, tmp_path):
    """the DataLoader collate (-> on_after_batch_transfer) and HostWaveSource: draws in the main process, f32 -> f32"""
    from lightning_asr_amd.data_module import LibriDataModule, load_wav
    from lightning_asr_amd.fused_fit import HostWaveSource
    ds, pcms = _six_wavs(tmp_path)
    man = str(tmp_path / "m.json")
    mans = _noise_and_rir_manifests(tmp_path)
    dm = LibriDataModule([man], man, man, list("abcdefg"), train_bs=3, dev_bs=3, num_worker=0, device=str(dev), train_crop=False,
                         speed_perturb=FACTORS, noise_manifest=mans["noise"], rir_manifest=mans["rir"], noise_prob=0.7, rir_prob=0.6,
                         noise_max_seconds=0.4)
    dm.setup()
    ap = dm.audio_parser
    wa = ap.wave_aug
    assert [c.size for c in wa.noises] == [900, 5500] and len(wa.rirs) == 3, "the budget cuts the bank in manifest order"
    op = wa.op()
    assert op.n_rir == 3 and op.noise_lens == [900, 5500]
    items = [dm.train_datasets[i] for i in range(3)]
    wb = dm._collate_train(items)
    assert wb.leads is None
    assert dm.draw_wave_aug_batch(3, False) is None                    # evaluation batches are never augmented
    dith = ap.device_dither()
    step0 = dith.step.clone()
    ap.rand = random.Random(21)                                        # factors, then parameter words, then the rectangles
    inputs, _, pct, _, _ = dm.on_after_batch_transfer(wb)
    ap.rand = random.Random(21)
    speed = dm.draw_speed_batch(3, True)
    words = dm.draw_wave_aug_batch(3, True)
    rs = ap.speed_resampler()
    singles = []
    for w, k, word in zip(wb[0], speed, words):
        out, n = rs(w.to(dev).unsqueeze(0), conv_id=torch.tensor([k], dtype=torch.int32, device=dev))
        x = out[:, :int(n[0])].contiguous()
        y, _, _ = op(x, None, torch.tensor([list(word)], dtype=torch.int32))
        if word[0] >= 0 or word[1] >= 0:
            _check_row(y[0].cpu().numpy(), x[0].cpu().numpy().astype(np.float64), word, wa, False)
        else:
            assert torch.equal(y, x)
        singles.append(y[0])
    dith.step.copy_(step0)
    want, want_pct = ap.features(singles, True)                        # (its rectangles continue the stream the draws came from)
    assert torch.equal(inputs, want) and torch.equal(pct, want_pct)
    # evaluation batches through the same hook are today's
    dith.step.copy_(step0)
    ev = dm.on_after_batch_transfer(dm._collate_eval(items))
    dith.step.copy_(step0)
    assert torch.equal(ev[0], ap.features([it[0] for it in items], False)[0])
    # HostWaveSource over the same loader
    ap.rand = random.Random(9)
    src = HostWaveSource(dm.train_dataloader(), dev, 2, audio_parser=ap)
    n_seen, kinds = 0, set()
    for db in src:
        assert db.speed is not None and db.wave_aug is not None and db.pcm.dtype == torch.float32
        files = {p: load_wav(p)[0] for p in db.paths}
        for i, p in enumerate(db.paths):
            n = ap.speed_out_len(files[p].numel(), db.speed[i])
            assert int(db.lens[i]) == n and not db.pcm[i, n:].any()
            one, _ = rs(files[p].to(dev).unsqueeze(0), conv_id=torch.tensor([db.speed[i]], dtype=torch.int32, device=dev))
            word = db.wave_aug[i]
            kinds.add((word[0] >= 0, word[1] >= 0))
            if word[0] < 0 and word[1] < 0:
                assert torch.equal(db.pcm[i, :n], one[0, :n])
            else:
                _check_row(db.pcm[i, :n].cpu().numpy(), one[0, :n].cpu().numpy().astype(np.float64), word, wa, False)
        assert db.L == int(db.lens.max()) and db.pcm.shape[1] == db.pitch
        n_seen += 1
    assert n_seen == 2 and len(kinds) >= 2
    for kw, key in ((dict(noise_prob=2), "noise_prob"), (dict(rir_prob=-1), "rir_prob"), (dict(noise_snr_db=[9, 3]), "noise_snr_db"),
                    (dict(noise_max_seconds=0), "noise_max_seconds")):
        with pytest.raises(ValueError, match=key):
            LibriDataModule([man], man, man, list("abcdefg"), device=str(dev), **kw)
    empty = tmp_path / "empty.json"
    empty.write_text("")
    with pytest.raises(ValueError, match="noise_manifest"):
        LibriDataModule([man], man, man, list("abcdefg"), device=str(dev), noise_manifest=str(empty)).setup()


def test_trainer_fit_with_every_augmentation_on(dev, tmp_path):
    from lightning_asr_amd.data_module import LibriDataModule
    from lightning_asr_amd.lightning_compat import Trainer, seed_everything
    from lightning_asr_amd.train import LightingModule
    data = tmp_path / "synth"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_data.py"), "--out", str(data), "--n-train", "12", "--n-dev", "4",
                    "--seconds", "2.0"], check=True)
    mans = _noise_and_rir_manifests(tmp_path)
    seed_everything(0)
    dm = LibriDataModule([str(data / "train.json")], str(data / "dev.json"), str(data / "dev.json"), LABELS, train_bs=4, dev_bs=4,
                         num_worker=2, device=str(dev), act_dtype=torch.bfloat16, speed_perturb=FACTORS, noise_manifest=mans["noise"],
                         rir_manifest=mans["rir"], noise_prob=0.7, rir_prob=0.6)
    model = LightingModule(learning_rate=1e-2, weight_decay=1e-3, labels=LABELS, total_epoch=1, drop_rate=0.0, mask=True, use_cer=True,
                           dtype="bf16", device=str(dev), warmup_steps=2)
    seen = []
    tr = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "run"), device=str(dev), check_val_every_n_epoch=1, log_every_n_steps=1)
    tr._fused_on_batch = lambda db: seen.append((db.speed, db.wave_aug, db.lens.clone(), db.pitch, db.L))
    hist = tr.fit(model, dm)
    assert tr.fused is not None and tr.fused.source_kind == "NativeSource" and tr.global_step == 3 and len(seen) == 3
    assert np.isfinite(hist[-1]["train_loss"]) and hist[-1]["train_loss"] > 0
    for speed, words, lens, pitch, L in seen:
        assert speed is not None and len(speed) == 4 and words is not None and len(words) == 4 and int(lens.max()) <= L < pitch
        assert all(int(n) < (1 << 30) for n in lens.tolist())           # no lead-in flags under augmentation
    kinds = set((w[0] >= 0, w[1] >= 0) for s in seen for w in s[1])
    assert len(kinds) >= 2
