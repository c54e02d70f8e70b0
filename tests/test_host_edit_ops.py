"""CPU tier of the edit alignment (substitutions / deletions / insertions behind the WER): the oracle's canonical script
(tests/helpers/edit_ops_oracle.py) against the properties every alignment has, the worked examples of the rule, the host path of
WER(detail=True), and the C ABI's exports and argument checks without a GPU."""
import ctypes
import os
import random
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import edit_ops_oracle as E  # noqa: E402


def test_oracle_script_properties():
    """4000 random pairs over a 3-letter vocabulary, lengths 0..8 (ties everywhere): the script costs exactly the Levenshtein
    distance of the library's host routine, consumes both sequences, and marks hits exactly where the units are equal"""
    from lightning_asr_amd.utils.asr_metrics import _edit_distance
    rng = random.Random(0)
    seen_ops = set()
    for _ in range(4000):
        h = [rng.randrange(3) for _ in range(rng.randrange(9))]
        r = [rng.randrange(3) for _ in range(rng.randrange(9))]
        d, ops = E.script(h, r)
        H, S, D, I = E.counts(ops)
        assert S + D + I == d == _edit_distance(h, r), (h, r, ops)
        assert H + S + D == len(r) and H + S + I == len(h), (h, r, ops)
        assert E.replay(h, r, ops), (h, r, ops)
        seen_ops.update(ops)
    assert seen_ops == {0, 1, 2, 3}
    assert not E.replay([1], [2], [0]) and not E.replay([1], [1], [1]) and not E.replay([1, 2], [1], [0])


def test_oracle_worked_examples():
    for h, r, want in [("ab", "ba", [1, 1]), ("a", "aa", [2, 0]), ("aa", "a", [3, 0]), ("abc", "bcd", [3, 0, 0, 2])]:
        assert E.script(list(h), list(r))[1] == want, (h, r)
    assert E.script([], []) == (0, [])
    assert E.script([], [5, 5]) == (2, [2, 2]) and E.script([5, 5], []) == (2, [3, 3])


def test_oracle_word_split_and_numpy_rows():
    assert E.words([0, 1, 2, 0, 0, 3, 0], 0) == [(1, 2), (3,)]            # leading, repeated and trailing spaces
    assert E.words([0, 0], 0) == [] and E.words([], 0) == []
    assert E.words([1, 2, 3], 9) == [(1, 2, 3)] and E.words([1, 0, 2], -1) == [1, 0, 2]
    rng = random.Random(1)
    for _ in range(50):                                                    # the long-case matrix against the plain one, cell for cell
        h = [rng.randrange(3) for _ in range(rng.randrange(30))]
        r = [rng.randrange(3) for _ in range(rng.randrange(30))]
        assert [list(map(int, row)) for row in E.matrix_np(h, r)] == E.matrix_py(h, r)
    h = [(1, 2), (3,), (1, 2)]                                             # units may be any hashable (words as tuples)
    assert [list(map(int, row)) for row in E.matrix_np(h, [(3,), (1, 2)])] == E.matrix_py(h, [(3,), (1, 2)])


def test_package_host_rule_is_the_oracle():
    """utils/asr_metrics._edit_ops (the package's own host function: it does not import the oracle) gives the oracle's script"""
    from lightning_asr_amd.utils.asr_metrics import _alignment, _edit_ops
    rng = random.Random(2)
    for _ in range(2000):
        h = [rng.randrange(3) for _ in range(rng.randrange(9))]
        r = [rng.randrange(3) for _ in range(rng.randrange(9))]
        assert _edit_ops(h, r) == E.script(h, r)[1], (h, r)
    assert _alignment(list("abc"), list("bcd"), [3, 0, 0, 2]) == [[None, "a", 3], ["b", "b", 0], ["c", "c", 0], ["d", None, 2]]
    for bad in ([0, 0, 0], [3, 0, 0], [3, 0, 0, 2, 2], [3, 1, 0, 2]):
        with pytest.raises(ValueError):
            _alignment(list("abc"), list("bcd"), bad)


def _ids_batch(rows, width, dtype):
    out = torch.zeros(len(rows), width, dtype=dtype)
    for b, row in enumerate(rows):
        out[b, :len(row)] = torch.tensor(row, dtype=dtype)
    return out


@pytest.mark.parametrize("use_cer", [False, True])
def test_wer_detail_host_path_matches_oracle(use_cer, monkeypatch):
    """a vocabulary with a multi-character label cannot take the device path: WER(detail=True) runs the same rule on the host.
    Only the greedy CTC collapse is a device routine; here the metric's decoding step is replaced by its definition (drop
    repeats, then blanks)."""
    from lightning_asr_amd.utils.asr_metrics import WER
    vocab = [" ", "a", "b", "<unk>"]
    blank = len(vocab)

    def collapse(ids):
        out, prev = [], -1
        for c in ids:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        return out

    def decode(predictions, predictions_len=None):
        return ["".join(vocab[c] for c in collapse(row)) for row in predictions.tolist()]
    wer = WER(vocab, use_cer=use_cer, detail=True)
    plain = WER(vocab, use_cer=use_cer)
    monkeypatch.setattr(wer, "ctc_decoder_predictions_tensor", decode)
    monkeypatch.setattr(plain, "ctc_decoder_predictions_tensor", decode)
    assert not wer.device_ok and wer.detail and not plain.detail
    rng = random.Random(3)
    want = [0] * 6
    for _ in range(2):                                               # two updates accumulate
        hyp_ids = [[rng.choice([0, 1, 2, 3, blank]) for _ in range(12)] for _ in range(5)]
        ref_ids = [[rng.randrange(4) for _ in range(rng.randrange(8))] for _ in range(5)]
        preds = torch.tensor(hyp_ids, dtype=torch.int64)
        targets = _ids_batch(ref_ids, 8, torch.int64)
        tl = torch.tensor([len(r) for r in ref_ids], dtype=torch.int64)
        wer.update(preds, targets, tl)
        plain.update(preds, targets, tl)
        assert not wer.device_path(preds, targets)
        for b in range(5):
            h = "".join(vocab[c] for c in collapse(hyp_ids[b]))
            r = "".join(vocab[c] for c in ref_ids[b])
            hu, ru = (list(h), list(r)) if use_cer else (h.split(), r.split())
            d, script = E.script(hu, ru)
            for k, v in enumerate([d, len(ru)] + E.counts(script)):
                want[k] += v
    got = wer.compute_detail()
    assert [got["hits"], got["subs"], got["dels"], got["ins"], got["ref_units"]] == want[2:] + [want[1]]
    assert got["subs"] + got["dels"] + got["ins"] == want[0] and want[1] > 0
    assert got["wer"] == pytest.approx(want[0] / want[1]) and got["sub_rate"] == pytest.approx(want[3] / want[1])
    assert got["del_rate"] == pytest.approx(want[4] / want[1]) and got["ins_rate"] == pytest.approx(want[5] / want[1])
    assert set(got) == {"wer", "sub_rate", "del_rate", "ins_rate", "hits", "subs", "dels", "ins", "ref_units"}
    assert float(wer.compute_total()) == pytest.approx(float(plain.compute_total())) == pytest.approx(got["wer"])
    with pytest.raises(RuntimeError):
        plain.compute_detail()
    wer.reset()
    assert wer.compute_detail()["ref_units"] == 0


def test_library_exports_edit_align_and_refuses_bad_calls_without_gpu():
    from lightning_asr_amd import _lib, ops
    lib = _lib.load()
    assert lib.lasr_version() >= 109
    assert hasattr(lib, "lasr_edit_align_batch") and hasattr(lib, "lasr_edit_align_workspace_bytes")
    assert "lasr_edit_align_batch" in _lib.SIGNATURES and "lasr_edit_align_workspace_bytes" in _lib.SIGNATURES
    E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
    ws_bytes = lib.lasr_edit_align_workspace_bytes
    assert ws_bytes(3, 501, 100) == 3 * 100 * 64 * 8 and ws_bytes(3, 100, 501) == ws_bytes(3, 501, 100)
    assert ws_bytes(1, 1, 1) == 512 and ws_bytes(0, 4, 4) == 0 and ws_bytes(1, 0, 4) == 0
    # host buffers stand in for device pointers: every call below is refused before anything is launched
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(ld_h=8, ld_r=4, B=1, space=-1, ld_ops=12, conf=None, n_classes=0, ws=p, ws_bytes_=None, ops_=p):
        need = ws_bytes(B, ld_h, ld_r) if ws_bytes_ is None else ws_bytes_
        return lib.lasr_edit_align_batch(p, p, ld_h, p, p, ld_r, B, space, p, p, p, ops_, ld_ops, p, None, conf, n_classes, ws, need, None)

    assert call(ops_=None) == E_ARG and b"null pointer" in lib.lasr_last_error()
    assert call(ws=None) == E_ARG
    assert call(ld_h=2049, ld_ops=4096) == E_SHAPE and b"2048" in lib.lasr_last_error()
    assert call(ld_r=2049, ld_ops=4096) == E_SHAPE
    assert call(ld_ops=11) == E_SHAPE and b"ld_ops" in lib.lasr_last_error()
    assert call(ws_bytes_=ws_bytes(1, 8, 4) - 1) == E_WORKSPACE and b"workspace" in lib.lasr_last_error()
    assert call(B=0) == E_SHAPE and call(ld_h=0) == E_SHAPE
    assert call(space=0, conf=p, n_classes=4) == E_ARG and b"confusion" in lib.lasr_last_error()
    assert call(conf=p, n_classes=0) == E_ARG
    # ops: CPU tensors are refused, never emulated; dtypes and shapes are checked before any launch
    tok, n = torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    tg, tl = torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.LasrError):
        ops.edit_ops_batch(tok, n, tg, tl)
    with pytest.raises(ValueError):
        ops.edit_ops_batch(tok.long(), n, tg, tl)
    with pytest.raises(ValueError):
        ops.edit_ops_batch(tok, n, tg.int(), tl)
    with pytest.raises(ValueError):
        ops.edit_ops_batch(tok, n.long(), tg, tl)
    with pytest.raises(TypeError):
        ops.edit_ops_batch(tok, n, tg, tl, totals=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.edit_ops_batch(tok, n, tg, tl, confusion=torch.zeros(3, 4, dtype=torch.int32))
    assert ops.EditOps._fields == ("dist", "ref_units", "counts", "ops", "n_ops")
