"""GPU tier, end to end: Trainer(pseudo_label=...) labels an unlabelled manifest between an epoch's training and its validation,
injects what passes into the training set and trains the next epoch on the enlarged set; AsrTranslator writes the same labels
as a manifest.  Smallest synthetic corpus, randomly initialised model."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = [c.strip() for c in open(os.path.join(ROOT, "data", "labels.txt")).readlines()]
N_TRAIN, N_UNL, BS = 8, 6, 4


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("pseudo")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_data.py"), "--out", str(d), "--n-train", str(N_TRAIN),
                    "--n-dev", str(N_UNL), "--seconds", "2.0"], check=True)
    unl = d / "unlabelled.json"                                   # the dev clips without their transcripts
    with open(d / "dev.json", encoding="utf-8") as f, open(unl, "w", encoding="utf-8") as g:
        for line in f:
            rec = json.loads(line)
            g.write(json.dumps({"audio_filepath": rec["audio_filepath"], "duration": rec["duration"]}) + "\n")
    return d


def _fit(dev, corpus, root, threshold, measure="ref"):
    from lightning_asr_amd.data_module import LibriDataModule
    from lightning_asr_amd.lightning_compat import Trainer, seed_everything
    from lightning_asr_amd.pseudo_label import PseudoLabelConfig
    from lightning_asr_amd.train import LightingModule
    seed_everything(0)
    dm = LibriDataModule([str(corpus / "train.json")], str(corpus / "dev.json"), str(corpus / "dev.json"), LABELS, train_bs=BS, dev_bs=BS,
                         num_worker=2, device=str(dev), act_dtype=torch.float32, pesudo_manifest=str(corpus / "unlabelled.json"))
    model = LightingModule(learning_rate=1e-3, weight_decay=1e-3, labels=LABELS, total_epoch=2, mask=True, use_cer=True, dtype="f32",
                           device=str(dev), warmup_steps=2)
    cfg = PseudoLabelConfig(manifest=str(corpus / "unlabelled.json"), start_epoch=0, every_n_epochs=1, threshold=threshold, measure=measure)
    tr = Trainer(max_epochs=2, default_root_dir=str(root), device=str(dev), pseudo_label=cfg, log_every_n_steps=1)
    rounds = []

    def hook(paths, logp, t_lens, gc, conf):
        texts = model.wer.ctc_decoder_predictions_tensor(logp.argmax(-1), t_lens)
        rounds.append({"epoch": tr.current_epoch, "paths": list(paths), "texts": list(texts), "n": gc.n_tokens.tolist(),
                       "conf": conf.tolist()})
    tr._pseudo_on_batch = hook
    sizes = []
    tr.callbacks.append(type("Sizes", (), {"on_train_batch_end": lambda self, t: sizes.append((t.current_epoch, len(dm.train_datasets)))})())
    hist = tr.fit(model, dm)
    records = [json.loads(line) for line in open(os.path.join(str(root), "metrics.jsonl"))]
    return tr, dm, hist, records, rounds, sizes


@pytest.mark.parametrize("measure", ["ref", "posterior"])
def test_fit_injects_every_labelled_utterance(dev, corpus, tmp_path, measure):
    tr, dm, hist, records, rounds, sizes = _fit(dev, corpus, tmp_path / "run", float("inf"), measure)
    assert len(hist) == 2 and len(records) == 2
    first = [r for r in rounds if r["epoch"] == 0]
    assert sum(len(r["paths"]) for r in first) == N_UNL
    # what the round after epoch 0 had to inject: every utterance with at least one token, with the decode of the SAME log-probs
    want = [(p, t) for r in first for p, t, n in zip(r["paths"], r["texts"], r["n"]) if n >= 1]
    assert all(len(t) == n for r in first for t, n in zip(r["texts"], r["n"]))
    # epoch 1 trained on original + injected: every batch of it saw the enlarged set, and there were len(loader) of them
    n1 = N_TRAIN + len(want)
    assert {s for e, s in sizes if e == 0} == {N_TRAIN} and {s for e, s in sizes if e == 1} == {n1}
    assert hist[0]["global_step"] == N_TRAIN // BS and hist[1]["global_step"] - hist[0]["global_step"] == n1 // BS
    assert records[0]["pseudo_seen"] == N_UNL and records[0]["pseudo_count"] == len(want)
    assert records[0]["pseudo_fraction"] == pytest.approx(len(want) / N_UNL)
    # the set now injected is the last round's (it replaced the first): its texts are that round's decodes
    last = [r for r in rounds if r["epoch"] == 1]
    want_last = [(p, t) for r in last for p, t, n in zip(r["paths"], r["texts"], r["n"]) if n >= 1]
    got = [(d["audio_filepath"], d["text"]) for d in dm.train_datasets.datasets[N_TRAIN:]]
    assert got == want_last and len(dm.train_dataloader().dataset) == N_TRAIN + len(want_last)
    assert records[1]["pseudo_count"] == len(want_last)
    assert len(want) > 0, "a randomly initialised model that decodes nothing cannot show the injection"


def test_fit_with_nothing_injected(dev, corpus, tmp_path):
    tr, dm, hist, records, rounds, sizes = _fit(dev, corpus, tmp_path / "run", -1.0)
    assert len(hist) == 2 and len(records) == 2                   # two whole epochs
    assert {s for _, s in sizes} == {N_TRAIN} and len(dm.train_datasets) == N_TRAIN and len(dm.train_dataloader()) == N_TRAIN // BS
    assert hist[1]["global_step"] == 2 * (N_TRAIN // BS)
    keys = ("pseudo_seen", "pseudo_count", "pseudo_fraction")
    for rec in records:
        assert all(k in rec for k in keys) or not any(k in rec for k in keys)
    rec = records[-1]                                             # written after a round that injected nothing
    assert rec["pseudo_seen"] == N_UNL and rec["pseudo_count"] == 0 and rec["pseudo_fraction"] == 0
    assert all(c > -1.0 for r in rounds for c in r["conf"])       # confidences are positive: none can pass -1


def test_translator_manifest_round_trip_and_confidence(dev, corpus, tmp_path):
    from lightning_asr_amd.data_module import MyAudioDataset
    from lightning_asr_amd.predict import AsrTranslator
    tr, dm, hist, records, rounds, sizes = _fit(dev, corpus, tmp_path / "run", -1.0)
    t = AsrTranslator(os.path.join(str(tmp_path / "run"), "checkpoints", "last.ckpt"), map_location=str(dev), labels=LABELS)
    out = tmp_path / "pseudo.json"
    stats = t.pseudo_label_manifest(str(corpus / "unlabelled.json"), str(out), threshold=float("inf"), batch_size=4, min_tokens=0)
    assert stats == {"pseudo_seen": N_UNL, "pseudo_count": N_UNL, "pseudo_fraction": 1.0}
    lines = [json.loads(line) for line in open(out, encoding="utf-8")]
    assert len(lines) == N_UNL and all(set(d) == {"audio_filepath", "duration", "text", "confidence"} for d in lines)
    ds = MyAudioDataset([str(out)], LABELS, mask=True)            # the file is a training manifest
    assert len(ds) == N_UNL
    for i, d in enumerate(lines):
        wave, ids, path = ds[i]
        assert path == d["audio_filepath"] and "".join(LABELS[k] for k in ids) == d["text"] and wave.numel() == 32000
    none = t.pseudo_label_manifest(str(corpus / "unlabelled.json"), str(tmp_path / "none.json"), threshold=-1.0)
    assert none["pseudo_count"] == 0 and open(tmp_path / "none.json").read() == ""
    uc = t.utterance_confidence(lines[0]["audio_filepath"])
    assert set(uc) == {"text", "ref", "nonblank", "posterior", "tokens"} and len(uc["tokens"]) == len(uc["text"])
    assert uc["posterior"] <= uc["ref"] + 1e-3 and uc["ref"] > 0
    for a, b in zip(uc["tokens"], uc["tokens"][1:]):
        assert 0 <= a["start"] < a["end"] <= b["start"] <= 2.0 + 1e-6 and a["min"] <= a["mean"] <= 0
    assert "".join(k["label"] for k in uc["tokens"]) == uc["text"]
