"""GPU tier of the edit alignment (csrc/editdist.hip edit_align_kernel, include/lasr.h lasr_edit_align_batch).  The alignment is
integer work with one canonical answer, so every case holds counts, the script and its length to the plain-Python oracle
(tests/helpers/edit_ops_oracle.py) EXACTLY, and dist / ref_units to ops.edit_distance_batch bit for bit: small vocabularies (ties
at almost every cell), every cells-per-lane template and its boundary, both orientations of the DP, word units, the totals and the
confusion matrix, refused calls, graph capture, and the Python surface (WER(detail=True), AsrTranslator.error_report)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import edit_ops_oracle as E  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 255


def rand_rows(rng, lens, vocab):
    return [rng.randint(0, vocab, size=n).tolist() for n in lens]


def mutate(rng, row, vocab, rate=0.2):
    """a noisy copy: substitutions, deletions and insertions at `rate` each"""
    out = []
    for t in row:
        u = rng.rand()
        if u < rate:
            out.append(int(rng.randint(0, vocab)))
        elif u < 2 * rate:
            continue
        else:
            out.append(t)
        if rng.rand() < rate:
            out.append(int(rng.randint(0, vocab)))
    return out


def pack(rows, width, dtype, fill=0):
    out = np.full((len(rows), width), fill, dtype=dtype)
    for b, row in enumerate(rows):
        out[b, :len(row)] = row
    return out


def run(dev, hyp_rows, ref_rows, space_id=-1, ld_h=None, ld_r=None, totals=None, confusion=None, hyp_lens=None, ref_lens=None):
    """ops.edit_ops_batch on padded rows -> numpy outputs, after the checks every case shares: exact agreement with the oracle and
    bit-equality of dist / ref_units with ops.edit_distance_batch on the same inputs.  The padding holds tokens the lengths must
    keep out of the result."""
    from lightning_asr_amd import ops
    ld_h = ld_h or max(1, max(len(r) for r in hyp_rows))
    ld_r = ld_r or max(1, max(len(r) for r in ref_rows))
    hyp = torch.from_numpy(pack(hyp_rows, ld_h, np.int32, fill=1)).to(dev)
    ref = torch.from_numpy(pack(ref_rows, ld_r, np.int64, fill=2)).to(dev)
    nh = torch.tensor([len(r) for r in hyp_rows] if hyp_lens is None else hyp_lens, dtype=torch.int32, device=dev)
    nr = torch.tensor([len(r) for r in ref_rows] if ref_lens is None else ref_lens, dtype=torch.int32, device=dev)
    res = ops.edit_ops_batch(hyp, nh, ref, nr, space_id, totals, confusion)
    dist, units = ops.edit_distance_batch(hyp, nh, ref, nr, space_id)
    torch.cuda.synchronize()
    assert res.ops.shape == (len(hyp_rows), ld_h + ld_r) and res.ops.dtype == torch.uint8 and res.counts.shape == (len(hyp_rows), 4)
    assert torch.equal(res.dist, dist) and torch.equal(res.ref_units, units)
    got = tuple(o.cpu().numpy() for o in res)
    want = E.align_batch(hyp.cpu().numpy(), nh.tolist(), ref.cpu().numpy(), nr.tolist(), space_id)
    for b, (d, n_ref, cnt, script, _, _) in enumerate(want):
        ctx = (b, len(hyp_rows[b]), len(ref_rows[b]))
        assert got[0][b] == d and got[1][b] == n_ref, (ctx, got[0][b], d, got[1][b], n_ref)
        assert got[4][b] == len(script), (ctx, got[4][b], len(script))
        assert got[3][b, :len(script)].tolist() == script, (ctx, got[3][b, :len(script)].tolist(), script)
        assert (got[3][b, len(script):] == PAD).all(), ctx
        assert got[2][b].tolist() == cnt, (ctx, got[2][b].tolist(), cnt)
    return got, want


def test_random_token_mode_with_ties_and_empty_sides(dev):
    rng = np.random.RandomState(0)
    hyp = rand_rows(rng, rng.randint(0, 41, size=16), 4)
    ref = rand_rows(rng, rng.randint(0, 41, size=16), 4)
    hyp[0], ref[1] = [], []                                     # an empty hypothesis: deletions only; an empty reference: insertions only
    hyp[2], ref[2] = [], []                                     # both empty
    hyp[3] = list(ref[3]) if ref[3] else [1, 2, 3]
    ref[3] = list(hyp[3])                                       # identical: hits only
    hyp[4], ref[4] = [0, 1], [1, 0]                             # the worked examples of the rule
    hyp[5], ref[5] = [0], [0, 0]
    hyp[6], ref[6] = [0, 0], [0]
    hyp[7], ref[7] = [0, 1, 2], [1, 2, 3]
    got, want = run(dev, hyp, ref, ld_h=40, ld_r=40)
    assert got[4][2] == 0 and got[0][2] == 0 and got[2][2].tolist() == [0, 0, 0, 0]
    assert got[2][0].tolist() == [0, 0, len(ref[0]), 0] and got[2][1].tolist() == [0, 0, 0, len(hyp[1])]
    assert got[2][3].tolist() == [len(ref[3]), 0, 0, 0]
    assert [want[b][3] for b in (4, 5, 6, 7)] == [[1, 1], [2, 0], [3, 0], [3, 0, 0, 2]]


# reference lengths round the cells-per-lane templates of the launch (max pitch <= 128: 2 per lane, <= 512: 8, else 32) against a
# hypothesis shorter and longer than the reference: 127 / 128 with 5 run on 2 cells per lane, 129 on 8; 512 with 30 on 8, 513 on 32
@pytest.mark.parametrize("n_ref,n_hyp", [(127, 5), (128, 5), (129, 5), (127, 140), (128, 140), (129, 140),
                                         (512, 30), (513, 30), (512, 600), (513, 600)])
def test_lane_and_template_boundaries(dev, n_ref, n_hyp):
    rng = np.random.RandomState(n_ref * 7 + n_hyp)
    ref = rand_rows(rng, [n_ref, n_ref, n_ref - 1, max(n_ref // 2, 1)], 4)
    hyp = [rand_rows(rng, [n_hyp], 4)[0], mutate(rng, ref[1], 4)[:n_hyp], rand_rows(rng, [n_hyp - 1], 4)[0], mutate(rng, ref[3], 4)[:n_hyp]]
    run(dev, hyp, ref, ld_h=n_hyp, ld_r=n_ref)


def test_full_width_2048(dev):
    rng = np.random.RandomState(5)
    ref = rand_rows(rng, [2048, 300], 4)
    hyp = [(mutate(rng, ref[0], 4) + rand_rows(rng, [2048], 4)[0])[:2048], rand_rows(rng, [1500], 4)[0]]
    assert len(hyp[0]) == 2048
    run(dev, hyp, ref, ld_h=2048, ld_r=2048)


def test_orientation_hypothesis_longer_and_roles_exchanged(dev):
    """the kernel lays the longer side along the wave, so 200 against 10 and 10 against 200 run in opposite orientations; the rule is
    stated on hypothesis / reference, so exchanging the roles is NOT a mirror image of the script: the deletion is still tried
    before the insertion"""
    rng = np.random.RandomState(11)
    long_rows = rand_rows(rng, [200, 200, 199, 150, 200, 64], 3)
    short_rows = rand_rows(rng, [10, 9, 10, 10, 1, 10], 3)
    run(dev, long_rows, short_rows, ld_h=200, ld_r=10)
    run(dev, short_rows, long_rows, ld_h=10, ld_r=200)
    # 200 against 150: cells where the deletion and the insertion tie (and the diagonal is out) lie on the walk, so the script of
    # the exchanged pair is not the mirror image; "aba" against "bab" is [3, 0, 0, 2] both ways round
    long_rows = rand_rows(rng, [200] * 7, 3) + [[0, 1, 0]]
    short_rows = rand_rows(rng, [150] * 7, 3) + [[1, 0, 1]]
    _, want_a = run(dev, long_rows, short_rows, ld_h=200, ld_r=150)
    _, want_b = run(dev, short_rows, long_rows, ld_h=150, ld_r=200)
    mirror = {0: 0, 1: 1, 2: 3, 3: 2}
    differs = 0
    for wa, wb in zip(want_a, want_b):
        assert wa[0] == wb[0]                                   # the distance is symmetric; the script is not
        differs += wa[3] != [mirror[o] for o in wb[3]]
    assert differs >= 2 and want_a[7][3] == want_b[7][3] == [3, 0, 0, 2]      # a blindly mirrored trace-back would fail these rows
    # equal lengths with the roles exchanged (the orientation is the same, the tie-break still distinguishes the sides)
    x = rand_rows(rng, [33, 64, 65], 3)
    y = rand_rows(rng, [33, 64, 65], 3)
    run(dev, x, y)
    run(dev, y, x)


def test_word_mode(dev):
    sp = 0
    hyp = [[0, 0, 1, 2, 0, 0, 3, 0],            # leading, repeated, trailing spaces: words (1 2) (3)
           [1, 2, 0, 3],                        # (1 2) (3)
           [1, 0, 2],                           # "a b" against "b a" as words: a tie, two substitutions
           [0, 0, 0],                           # spaces only: no word
           [1, 2, 3, 0, 1, 2, 3, 0, 2],         # a repeated word
           [2, 1, 0, 1, 2],                     # the same ids in another order are another word
           []]
    ref = [[1, 2, 0, 3],
           [0, 1, 2, 0, 0, 4, 0, 3, 0],
           [2, 0, 1],
           [1, 0, 1],
           [1, 2, 3, 0, 2],
           [1, 2, 0, 1, 2],
           [0, 1, 0]]
    got, want = run(dev, hyp, ref, space_id=sp)
    assert want[0][3] == [0, 0] and want[2][3] == [1, 1] and want[3][3] == [2, 2] and want[1][3] == [0, 2, 0]
    assert got[1].tolist() == [2, 3, 2, 2, 2, 2, 1]
    # a space id beyond the vocabulary: one word per utterance (none for an empty one)
    got, want = run(dev, hyp, ref, space_id=7)
    assert got[1].tolist() == [1] * 7 and got[4].tolist() == [1, 1, 1, 1, 1, 1, 1]
    assert want[6][3] == [2] and want[3][3] == [1]
    # random word streams over a 2-letter alphabet: many equal words, many ties
    rng = np.random.RandomState(3)
    hyp = rand_rows(rng, rng.randint(0, 120, size=8), 3)
    ref = rand_rows(rng, rng.randint(0, 120, size=8), 3)
    run(dev, hyp, ref, space_id=0, ld_h=130, ld_r=120)


def test_lengths_are_clamped_to_the_pitches(dev):
    hyp = [[1, 2, 3, 1], [2, 2, 2, 2]]
    ref = [[1, 3, 3], [2, 1, 2]]
    run(dev, hyp, ref, hyp_lens=[9, -3], ref_lens=[3, 1000])


def test_totals_and_confusion_accumulate(dev):
    from lightning_asr_amd import ops
    n_cls = 4
    rng = np.random.RandomState(7)
    totals = torch.zeros(6, dtype=torch.int64, device=dev)
    conf = torch.zeros(n_cls + 1, n_cls + 1, dtype=torch.int32, device=dev)
    want_tot = np.zeros(6, np.int64)
    want_conf = np.zeros((n_cls + 1, n_cls + 1), np.int64)
    n_all = 0
    for call in range(2):
        # ids n_cls and -1 sit outside [0, n_cls): their ops are left out of the matrix, never written out of bounds
        hyp = [[int(t) for t in rng.randint(-1, n_cls + 1, size=n)] for n in rng.randint(0, 90, size=6)]
        ref = [[int(t) for t in rng.randint(-1, n_cls + 1, size=n)] for n in rng.randint(0, 70, size=6)]
        got, want = run(dev, hyp, ref, totals=totals, confusion=conf)
        for d, n_ref, cnt, script, _, _ in want:
            want_tot += np.array([d, n_ref] + cnt)
            n_all += len(script)
        want_conf += np.array(E.confusion(want, n_cls))
    torch.cuda.synchronize()
    assert totals.cpu().numpy().tolist() == want_tot.tolist()
    assert conf.cpu().numpy().tolist() == want_conf.tolist()
    assert 0 < int(want_conf.sum()) < n_all and want_conf[n_cls, n_cls] == 0
    assert want_conf[n_cls, :n_cls].sum() > 0 and want_conf[:n_cls, n_cls].sum() > 0 and np.trace(want_conf) > 0
    # either output alone
    hyp, ref = [[0, 1, 2, 3]], [[1, 2, 3, 3, 0]]
    t2 = torch.full((6,), 10, dtype=torch.int64, device=dev)
    _, want = run(dev, hyp, ref, totals=t2)
    assert t2.tolist() == [10 + v for v in [want[0][0], want[0][1]] + want[0][2]]
    c2 = torch.zeros(n_cls + 1, n_cls + 1, dtype=torch.int32, device=dev)
    _, want = run(dev, hyp, ref, confusion=c2)
    assert c2.cpu().numpy().tolist() == E.confusion(want, n_cls) and int(c2.sum()) == len(want[0][3])
    # the matrix is over token ids: refused with word units, and nothing is added
    before = c2.clone()
    with pytest.raises(Exception, match="confusion"):
        ops.edit_ops_batch(torch.zeros(1, 4, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev),
                           torch.zeros(1, 4, dtype=torch.int64, device=dev), torch.ones(1, dtype=torch.int32, device=dev), 0, None, c2)
    torch.cuda.synchronize()
    assert torch.equal(c2, before)


def test_bad_arguments_launch_nothing(dev):
    from lightning_asr_amd import _lib
    lib = _lib.load()
    E_SHAPE, E_WORKSPACE = -2, -3
    B = 2
    hyp = torch.zeros(B, 2049, dtype=torch.int32, device=dev)
    ref = torch.zeros(B, 2049, dtype=torch.int64, device=dev)
    lens = torch.full((B,), 8, dtype=torch.int32, device=dev)
    outs = {k: torch.full((n,), -77, dtype=torch.int32, device=dev) for k, n in
            (("dist", B), ("units", B), ("counts", 4 * B), ("n_ops", B), ("ops", B * 4100 // 4), ("ws", 1 << 16))}
    totals = torch.full((6,), -77, dtype=torch.int64, device=dev)
    conf = torch.full((25,), -77, dtype=torch.int32, device=dev)

    def call(ld_h, ld_r, ld_ops, ws_bytes):
        return lib.lasr_edit_align_batch(hyp.data_ptr(), lens.data_ptr(), ld_h, ref.data_ptr(), lens.data_ptr(), ld_r, B, -1,
                                         outs["dist"].data_ptr(), outs["units"].data_ptr(), outs["counts"].data_ptr(), outs["ops"].data_ptr(),
                                         ld_ops, outs["n_ops"].data_ptr(), totals.data_ptr(), conf.data_ptr(), 4, outs["ws"].data_ptr(),
                                         ws_bytes, torch.cuda.current_stream().cuda_stream)

    need = lib.lasr_edit_align_workspace_bytes(B, 16, 8)
    assert need == B * 8 * 512
    assert call(2049, 8, 4100, 1 << 18) == E_SHAPE and call(16, 2049, 4100, 1 << 18) == E_SHAPE
    assert call(16, 8, 24, need - 1) == E_WORKSPACE
    assert call(16, 8, 23, need) == E_SHAPE
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert (v == -77).all(), k
    assert (totals == -77).all() and (conf == -77).all()
    assert call(16, 8, 24, need) == 0                           # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert (outs["n_ops"] == 8).all() and (outs["dist"] == 0).all() and totals.tolist() == [-77, 16 - 77, 16 - 77, -77, -77, -77]


def test_deterministic_and_graph_capture(dev):
    from lightning_asr_amd import ops
    rng = np.random.RandomState(13)
    ref_rows = rand_rows(rng, [100, 80, 0, 100], 4)
    hyp_rows = [mutate(rng, ref_rows[0], 4), rand_rows(rng, [300], 4)[0], rand_rows(rng, [17], 4)[0], []]
    _, want = run(dev, hyp_rows, ref_rows, ld_h=300, ld_r=100)
    hyp = torch.from_numpy(pack(hyp_rows, 300, np.int32)).to(dev)
    ref = torch.from_numpy(pack(ref_rows, 100, np.int64)).to(dev)
    nh = torch.tensor([len(r) for r in hyp_rows], dtype=torch.int32, device=dev)
    nr = torch.tensor([len(r) for r in ref_rows], dtype=torch.int32, device=dev)
    a = ops.edit_ops_batch(hyp, nh, ref, nr)
    totals = torch.zeros(6, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.edit_ops_batch(hyp, nh, ref, nr, -1, totals)
    torch.cuda.current_stream().wait_stream(s)
    totals.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = ops.edit_ops_batch(hyp, nh, ref, nr, -1, totals)
    for _ in range(2):
        for o in c:
            o.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        for u, v in zip(a, c):
            assert torch.equal(u, v)
    one = [sum(w[0] for w in want), sum(w[1] for w in want)] + [sum(w[2][k] for w in want) for k in range(4)]
    assert totals.tolist() == [2 * v for v in one]              # the graph's own accumulation: once per replay


@pytest.mark.parametrize("use_cer", [False, True])
def test_wer_detail_on_device_tensors(dev, use_cer):
    from lightning_asr_amd.utils.asr_metrics import WER
    vocab = [" ", "a", "b", "c"]
    blank = len(vocab)
    wer, plain = WER(vocab, use_cer=use_cer, detail=True), WER(vocab, use_cer=use_cer)
    assert wer.device_ok
    rng = np.random.RandomState(17)
    want = np.zeros(6, np.int64)
    for _ in range(2):
        B, T, S = 6, 50, 20
        preds = torch.from_numpy(rng.randint(0, blank + 1, size=(B, T))).to(dev)
        t_lens = torch.from_numpy(rng.randint(0, T + 1, size=B).astype(np.int32)).to(dev)
        targets = torch.from_numpy(rng.randint(0, blank, size=(B, S))).to(dev)
        tl = torch.from_numpy(rng.randint(0, S + 1, size=B)).to(dev)
        assert wer.device_path(preds, targets)
        batch = wer(preds, targets, tl, t_lens)
        assert float(batch) == float(plain(preds, targets, tl, t_lens)) or (math.isnan(float(batch)) and math.isnan(float(plain.compute())))
        p = preds.cpu().numpy()
        for b in range(B):
            ids, prev = [], -1
            for c in p[b, :int(t_lens[b])]:
                if c != prev and c != blank:
                    ids.append(int(c))
                prev = c
            h = "".join(vocab[c] for c in ids)
            r = "".join(vocab[c] for c in targets[b, :int(tl[b])].tolist())
            hu, ru = (list(h), list(r)) if use_cer else (h.split(), r.split())
            d, script = E.script(hu, ru)
            want += np.array([d, len(ru)] + E.counts(script))
    got = wer.compute_detail()
    assert [got["subs"] + got["dels"] + got["ins"], got["ref_units"], got["hits"], got["subs"], got["dels"], got["ins"]] == want.tolist()
    assert got["wer"] == want[0] / want[1] and got["sub_rate"] == want[3] / want[1]
    assert got["del_rate"] == want[4] / want[1] and got["ins_rate"] == want[5] / want[1]
    assert float(wer.compute_total()) == float(plain.compute_total()) == pytest.approx(want[0] / want[1], rel=1e-6)
    wer.world_reduce = lambda s, w: (2 * s, 2 * w)                # two ranks with the same data
    doubled = wer.compute_detail()
    assert doubled["hits"] == 2 * got["hits"] and doubled["ins"] == 2 * got["ins"] and doubled["wer"] == got["wer"]


# ------------------------------------------------------------------------------------------------ AsrTranslator.error_report
def _translator_fixture(tmp_path, use_cer):
    """the synthetic reference-style checkpoint and wavs of tests/test_gpu_ctc_align.py, with a manifest"""
    import wave as wavmod
    from oracle import ref_cpu as R
    from lightning_asr_amd.predict import EN_LABELS
    state = R.formula_state("plain", 29)
    for k_ in state:
        if k_.endswith("running_var"):
            state[k_] = state[k_] * 0 + 0.5 + 0.01 * torch.arange(state[k_].numel()).float() % 1.0
    ckpt = {"state_dict": {"encoder." + k_: v for k_, v in state.items()},
            "hyper_parameters": {"learning_rate": 1e-2, "weight_decay": 1e-3, "labels": EN_LABELS, "total_epoch": 1, "drop_rate": 0.0,
                                 "mask": True, "use_cer": use_cer}, "epoch": 0, "global_step": 0}
    path = tmp_path / "ref_style.ckpt"
    torch.save(ckpt, path)
    man = tmp_path / "m.json"
    texts = ("a b", "it's a test", "hello world")
    with open(man, "w") as f:
        for i, secs in enumerate((2.0, 1.5, 2.5)):
            g = torch.Generator().manual_seed(5 + i)
            n = int(16000 * secs)
            t = torch.arange(n) / 16000.0
            y = 0.3 * torch.sin(2 * math.pi * (220 + 60 * i + 180 * t) * t) + 0.05 * torch.randn(n, generator=g)
            pcm = (y.clamp(-1, 1) * 32767).to(torch.int16)
            wp = tmp_path / ("a%d.wav" % i)
            with wavmod.open(str(wp), "wb") as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.numpy().tobytes())
            f.write(json.dumps({"audio_filepath": str(wp), "duration": secs, "text": texts[i]}) + "\n")
    return str(path), str(man), texts


@pytest.mark.parametrize("decoder,use_cer", [("greedy", False), ("beam", False), ("greedy", True), ("beam", True)])
def test_error_report(dev, tmp_path, decoder, use_cer):
    from lightning_asr_amd.predict import AsrTranslator
    ckpt, man, texts = _translator_fixture(tmp_path, use_cer)
    tr = AsrTranslator(ckpt, map_location="cuda", decoder=decoder, beam_width=8)
    out_path = tmp_path / "errors.jsonl"
    summary = tr.error_report(man, str(out_path), batch_size=2, top=5)
    lines = [json.loads(l) for l in open(out_path, encoding="utf-8") if l.strip()]
    assert len(lines) == 3 == summary["utterances"] and sorted(l["ref"] for l in lines) == sorted(texts)
    tot = dict.fromkeys(("dist", "hits", "subs", "dels", "ins"), 0)
    units = 0
    pairs = {1: {}, 2: {}, 3: {}}
    for l in lines:
        assert set(l) == {"audio_filepath", "ref", "hyp", "dist", "hits", "subs", "dels", "ins", "alignment"}
        hu, ru = (list(l["hyp"]), list(l["ref"])) if use_cer else (l["hyp"].split(), l["ref"].split())
        script = [op for _, _, op in l["alignment"]]
        assert E.replay(hu, ru, script)                                     # the alignment replays hyp into ref ...
        assert [h for _, h, op in l["alignment"] if op != 2] == hu and [r for r, _, op in l["alignment"] if op != 3] == ru
        assert all((r is None) == (op == 3) and (h is None) == (op == 2) for r, h, op in l["alignment"])
        assert script == E.script(hu, ru)[1]                                # ... and is the canonical one
        assert [l["hits"], l["subs"], l["dels"], l["ins"]] == E.counts(script) and l["dist"] == l["subs"] + l["dels"] + l["ins"]
        for k in tot:
            tot[k] += l[k]
        units += len(ru)
        for r, h, op in l["alignment"]:
            if op:
                pairs[op][(r, h)] = pairs[op].get((r, h), 0) + 1
    assert {k: summary[k] for k in tot} == tot and summary["ref_units"] == units and summary["use_cer"] == use_cer
    assert summary["wer"] == tot["dist"] / units and summary["sub_rate"] == tot["subs"] / units
    assert summary["del_rate"] == tot["dels"] / units and summary["ins_rate"] == tot["ins"] / units
    # the confusion lists (over characters: read from the device matrix) are the scripts' own pairs, most frequent first
    assert len(summary["top_substitutions"]) == min(5, len(pairs[1])) and len(summary["top_deletions"]) == min(5, len(pairs[2]))
    for r, h, v in summary["top_substitutions"]:
        assert pairs[1][(r, h)] == v
    for r, v in summary["top_deletions"]:
        assert pairs[2][(r, None)] == v
    for h, v in summary["top_insertions"]:
        assert pairs[3][(None, h)] == v
    for key in ("top_substitutions", "top_deletions", "top_insertions"):
        assert [e[-1] for e in summary[key]] == sorted((e[-1] for e in summary[key]), reverse=True)
    if pairs[1]:
        assert summary["top_substitutions"][0][2] == max(pairs[1].values())
    # the same WER as evalute_manifest's epoch: its summed distances over its summed reference units
    outs = tr.evalute_manifest(man, batch_size=2, decoder=decoder)
    preds = [p for o in outs for p in o["pred"]]
    trues = [t for o in outs for t in o["true"]]
    by_ref = {l["ref"]: l["hyp"] for l in lines}
    assert [by_ref[t] for t in trues] == preds
    from lightning_asr_amd.utils.asr_metrics import word_error_rate
    assert summary["wer"] == pytest.approx(word_error_rate(preds, trues, use_cer=use_cer), abs=1e-9)
