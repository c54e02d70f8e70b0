"""Host tier of pseudo-label self-training: the confidence oracle against the reference's recorded outputs, the round schedule, and
the data module's unlabelled manifest and injection.  No GPU."""
import json
import os
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import greedy_conf_oracle as O  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "pseudo_confidence.npz")
LABELS = [c.strip() for c in open(os.path.join(ROOT, "data", "labels.txt")).readlines()]


def golden_cases():
    g = np.load(GOLD)
    for name in g["cases"]:
        seed, B, T, C = (int(v) for v in g[name + "_shape"])
        yield str(name), seed, B, T, C, float(g[name + "_blank_bias"]), g[name + "_lens"], g[name + "_sum_logprob"], g[name + "_seq_sum_logprob_np"]


def test_oracle_matches_the_reference_confidences():
    """conf[0] of the oracle is the reference's value: against sum_logprob (Python-float sums) to T * 2^-52 relative - the terms
    share a sign, so the exact sum and a sequential f64 sum differ by at most that - and against seq_sum_logprob_np (whose
    running sum is f32) to T * 2^-24."""
    names = []
    for name, seed, B, T, C, bias, lens, want64, want32 in golden_cases():
        names.append(name)
        logp = O.make_logp(seed, B, T, C, C - 1, bias)
        o = O.oracle(logp, lens, C - 1)
        assert (o["n_nonblank"] < np.minimum(lens, T)).any(), "the case must hold frames where the blank wins"
        assert (lens < T).any()
        e64, e32 = O.rel_err(o["conf"][:, 0], want64), O.rel_err(o["conf"][:, 0], want32)
        print(name, "rel err vs sum_logprob %.3g, vs seq_sum_logprob_np %.3g" % (e64, e32))
        assert e64 <= T * 2.0 ** -52
        assert e32 <= T * 2.0 ** -24
        # the label-frames-only measure differs wherever the blank won: the reference's `index == vocab_size` never fires
        assert not np.allclose(o["conf"][:, 0], o["conf"][:, 1])
    assert sorted(names) == ["c28", "c4334"]


def test_oracle_constructed_rows():
    ninf = -np.inf
    blank = 3
    lp = np.full((1, 7, 4), -5.0, np.float32)
    for t, c in enumerate([1, 1, 3, 1, 2, 2, 0]):       # label - blank - same label: two tokens; then a two-frame run; padding
        lp[0, t, c] = -0.5 - 0.25 * t
    lp[0, 6] = 100.0                                     # past lens: must not leak
    o = O.oracle(lp, [6], blank)
    assert o["n_tokens"][0] == 3 and o["tokens"][0, :4].tolist() == [1, 1, 2, -1]
    assert o["tok_start"][0, :3].tolist() == [0, 3, 4] and o["tok_end"][0, :3].tolist() == [2, 4, 6]
    assert o["tok_min"][0, 0] == np.float32(-0.75) and o["tok_mean"][0, 2] == (-1.5 - 1.75) / 2
    assert o["n_nonblank"][0] == 5 and o["utt_sum"][0, 0] == sum(-0.5 - 0.25 * t for t in range(6))
    tie = np.array([[[-1.0, -1.0, -2.0, -1.0]]], np.float32)      # ties go to the lowest id
    assert O.oracle(tie, None, blank)["tokens"][0, 0] == 0
    assert O.oracle(np.full((1, 2, 4), ninf, np.float32), None, 0)["n_tokens"][0] == 0      # rows of -inf: class 0 = the blank here
    empty = O.oracle(lp, [0], blank)
    assert empty["conf"][0].astype(np.float32).tolist() == [10.0, 10.0]       # (1e-5 / 1e-6 is 10 to an f64 ulp)
    assert empty["n_tokens"][0] == 0


def test_round_due_truth_table():
    from lightning_asr_amd.pseudo_label import PseudoLabelConfig, round_due
    cfg = PseudoLabelConfig(manifest="x.json")
    assert (cfg.start_epoch, cfg.every_n_epochs, cfg.threshold, cfg.measure, cfg.min_tokens, cfg.batch_size) == (300, 7, 0.01, "ref", 1, None)
    got = {e: round_due(e, cfg) for e in (0, 299, 300, 301, 307, 308)}
    assert got == {0: False, 299: False, 300: False, 301: True, 307: False, 308: True}      # 301 = 43 * 7, 308 = 44 * 7
    assert round_due(0, PseudoLabelConfig(manifest="x", start_epoch=0, every_n_epochs=1)) and \
        round_due(5, PseudoLabelConfig(manifest="x", start_epoch=0, every_n_epochs=1))
    with pytest.raises(ValueError):
        PseudoLabelConfig(manifest="x", measure="beam")


def _wav(path, seconds):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.arange(int(16000 * seconds)) % 50).astype("<i2").tobytes())
    return str(path)


def _manifest(path, items):
    with open(path, "w", encoding="utf-8") as f:
        for it in items:
            f.write(json.dumps(it) + "\n")
    return str(path)


@pytest.fixture()
def corpus(tmp_path):
    train = [{"audio_filepath": _wav(tmp_path / ("t%d.wav" % i), 0.1), "duration": 0.1, "text": "ab"} for i in range(3)]
    unl = [{"audio_filepath": _wav(tmp_path / ("u%d.wav" % i), 0.1 if i < 3 else 0.5), "duration": 0.1 if i < 3 else 0.5} for i in range(4)]
    unl.append({"audio_filepath": _wav(tmp_path / "u_far_too_long.wav", 0.1), "duration": 50.0})      # over dev_max_duration: not loaded
    return {"train": _manifest(tmp_path / "train.json", train), "unl": _manifest(tmp_path / "unl.json", unl),
            "train_items": train, "unl_items": unl, "dir": tmp_path}


def _dm(corpus, **kw):
    from lightning_asr_amd.data_module import LibriDataModule
    dm = LibriDataModule([corpus["train"]], corpus["train"], corpus["train"], LABELS, train_bs=2, dev_bs=2, num_worker=0, device="cpu",
                         train_max_duration=0.3, dev_max_duration=40, **kw)
    dm.setup("fit")
    return dm


def test_unlabelled_manifest_loads_for_the_pseudo_set_only(corpus):
    from lightning_asr_amd.data_module import MyAudioDataset
    dm = _dm(corpus, pesudo_manifest=corpus["unl"])
    ds = dm.pesudo_train_datasets
    assert len(ds) == 4 and all(d["text"] == "" for d in ds.datasets)        # cut at dev_max_duration, missing text = ""
    wave_, ids, path = ds[0]
    assert ids == [] and path == corpus["unl_items"][0]["audio_filepath"] and wave_.numel() == 1600
    loader = dm.pseudo_train_dataloader()
    assert len(loader) == 2 and [p for b in loader for p in b[3]] == [d["audio_filepath"] for d in corpus["unl_items"][:4]]   # no shuffle
    with pytest.raises(KeyError):                                            # the training set still needs its transcripts
        MyAudioDataset([corpus["unl"]], LABELS, mask=True)[0]
    plain = _dm(corpus)
    assert plain.pesudo_train_datasets is None
    with pytest.raises(RuntimeError):
        plain.pseudo_train_dataloader()


def test_inject_pesudo_datasets(corpus, caplog):
    dm = _dm(corpus, pesudo_manifest=corpus["unl"])
    u = [d["audio_filepath"] for d in corpus["unl_items"]]
    assert len(dm.train_dataloader().dataset) == 3 and len(dm.train_dataloader()) == 1
    # the reference's form: (path, text) pairs; a missing file and a clip over train_max_duration (0.5 s > 0.3 s) are dropped
    with caplog.at_level("WARNING"):
        n = dm.inject_pesudo_datasets([(u[0], "ab"), (str(corpus["dir"] / "gone.wav"), "a"), (u[3], "b"), (u[1], "")])
    assert n == 2 and "gone.wav" in caplog.text
    ds = dm.train_dataloader().dataset
    assert len(ds) == 5 and len(dm.train_dataloader()) == 2
    assert [(d["audio_filepath"], d["text"], d["duration"]) for d in ds.datasets[3:]] == [(u[0], "ab", 0.1), (u[1], "", 0.1)]
    assert ds[3][1] == [LABELS.index("a"), LABELS.index("b")]
    # label_loader's form: dicts; the new round REPLACES the previous one
    n = dm.inject_pesudo_datasets([{"audio_filepath": u[2], "duration": 0.1, "text": "b", "confidence": 0.001}])
    ds = dm.train_dataloader().dataset
    assert n == 1 and len(ds) == 4 and ds.datasets[3]["audio_filepath"] == u[2] and ds.datasets[:3] == corpus["train_items"]
    assert dm.inject_pesudo_datasets([]) == 0 and len(dm.train_dataloader().dataset) == 3
