"""Long transcripts (S_max > 511): the multi-wave CTC lattice of both loss heads against torch's CPU ctc_loss, its bit-identity
with the one-wave kernels, and validation over a manifest holding a 40 s clip (the reference's dev_max_duration)."""
import math
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _labels(B, W, lens, C, g, repeats):
    tg = torch.randint(0, C - 1, (B, W), generator=g)
    if repeats:
        tg[:, 1::5] = tg[:, 0::5][:, :tg[:, 1::5].shape[1]]           # adjacent repeats
    for b in range(B):
        tg[b, lens[b]:] = 0
    return tg


def _torch_ref(lp, tg, il, tl, gs):
    """torch's CPU ctc_loss in f64 (zero_infinity=False): per-sample nll and d(sum_b gs_b nll_b)/d logp"""
    lpr = lp.double().clone().requires_grad_(True)
    ref = F.ctc_loss(lpr.transpose(0, 1), tg, il.long(), tl.long(), blank=lp.shape[2] - 1, reduction="none", zero_infinity=False)
    ok = torch.isfinite(ref)
    (ref[ok] * gs.double()[ok]).sum().backward()
    return ref.detach(), lpr.grad, ok


def _torch_f32_err(lp, tg, il, tl, gs, ok, r):
    lpr = lp.float().clone().requires_grad_(True)
    ref = F.ctc_loss(lpr.transpose(0, 1), tg, il.long(), tl.long(), blank=lp.shape[2] - 1, reduction="none", zero_infinity=False)
    (ref[ok] * gs.float()[ok]).sum().backward()
    g = lpr.grad[ok].double()
    return float((g - r).abs().max() / r.abs().max()), rel_l2(g, r)


def _check(lp, tg, il, tl, dev, gs=None):
    from lightning_asr_amd import ops
    B = lp.shape[0]
    gs = torch.rand(B, generator=torch.Generator().manual_seed(1)) + 0.5 if gs is None else gs
    ref, gref, ok = _torch_ref(lp, tg, il, tl, gs)
    nll, grad = ops.ctc_loss(lp.to(dev), tg.to(dev), il.to(dev), tl.to(dev), lp.shape[2] - 1, True, gs.to(dev))
    nll, grad = nll.cpu(), grad.cpu()
    assert torch.equal(torch.isfinite(nll), ok), (nll, ref)
    assert ((nll.double()[ok] - ref[ok]).abs() / ref[ok].abs().clamp_min(1e-30)).max() < 1e-4, (nll, ref)
    for b in range(B):
        if not ok[b]:
            assert torch.isinf(nll[b]) and nll[b] > 0
            assert torch.isnan(grad[b, :int(il[b])]).all() and torch.all(grad[b, int(il[b]):] == 0)
    g, r = grad[ok].double(), gref[ok]
    # Gradient gates: the existing 2e-3, or twice what torch's own f32 ctc_loss reaches on the same batch, whichever is larger.
    # The occupancy exp(alpha + beta + nll - lp) of an f32 lattice loses what one ulp of |alpha| ~ nll is worth: random
    # log-probs give nll ~ T' log C (4e3 - 1.4e4 here), where f32 CTC in any implementation misses 2e-3.
    max_f, l2_f = _torch_f32_err(lp, tg, il, tl, gs, ok, r)
    err_max, err_l2 = float((g - r).abs().max() / r.abs().max()), rel_l2(g, r)
    print("GATES", tuple(lp.shape), err_max, err_l2, "torch f32:", max_f, l2_f)
    assert err_max < max(2e-3, 2 * max_f) + 1e-6, (err_max, max_f)
    assert err_l2 < max(2e-3, 2 * l2_f), (err_l2, l2_f)
    return nll, grad


# (S width, T', C): C = 28 with the emission rows in LDS where (T'+2)*C*4 fits beside the label table, C = 29 (rows not 16-byte
# multiples) on the register ring, and the AISHELL vocabulary on the ring
@pytest.mark.parametrize("S,T,C", [(512, 1100, 28), (600, 1300, 28), (600, 2001, 28), (1023, 2001, 29), (1024, 2200, 28),
                                   (1500, 2001, 29), (2047, 4100, 28), (600, 1250, 4334)])
def test_long_lattice_matches_torch(dev, S, T, C):
    g = torch.Generator().manual_seed(S * 7 + T)
    B = 4
    lp = F.log_softmax(torch.randn(B, T, C, generator=g) * 2, -1)
    tl = torch.tensor([S, S - 37, max(S // 3, 1), 0], dtype=torch.int32)      # ragged, and an empty target
    il = torch.tensor([T, T - 11, max(2 * S // 3 + 2, 1), T // 2], dtype=torch.int32)
    tg = _labels(B, S, tl.tolist(), C, g, repeats=True)
    _check(lp, tg, il, tl, dev)


def test_long_lattice_tight_infeasible_and_blank_dominated(dev):
    g = torch.Generator().manual_seed(5)
    B, S, C = 4, 700, 28
    tl = torch.tensor([S, 650, 600, S], dtype=torch.int32)
    tg = (torch.arange(S) % (C - 1)).repeat(B, 1)                      # no adjacent repeats: S frames suffice
    for b in range(B):
        tg[b, int(tl[b]):] = 0
    tg[2, 10] = tg[2, 11] = tg[2, 12]                                  # a short run of repeats (+2 frames)
    il = torch.tensor([S, 649, 602, 1400], dtype=torch.int32)          # tight; infeasible (649 < 650); tight with repeats; long
    T = 1400
    x = torch.randn(B, T, C, generator=g)
    x[3, :, C - 1] += 6.0                                              # blank-dominated utterance
    lp = F.log_softmax(x, -1)
    nll, _ = _check(lp, tg, il, tl, dev)
    assert torch.isinf(nll[1]) and torch.isfinite(nll[[0, 2, 3]]).all()


def _peaked(B, T, C, tg, tl, il, g):
    """log-probs concentrated on one feasible alignment per utterance (labels spread evenly, blanks between): |nll| stays modest
    (tens of nats), so the f32 lattice meets the strict 2e-3 gradient gate"""
    x = torch.randn(B, T, C, generator=g) * 0.5
    scale = 5.0 + math.log(C / 28.0)                                   # the path class at ~0.85 probability for any C
    for b in range(B):
        n, S = int(il[b]), int(tl[b])
        cls = torch.full((n,), C - 1, dtype=torch.long)
        if S:
            pos = (torch.arange(S) * n) // S
            cls[pos] = tg[b, :S]
        x[b, torch.arange(n), cls] += scale
    return F.log_softmax(x, -1)


# widths up to the reference's dev shape (T' <= 2001): 2 waves (states into wave 1 at S = 1000), 4 waves at S = 1536, the AISHELL
# vocabulary on the ring
@pytest.mark.parametrize("S,T,C", [(600, 1300, 28), (1000, 2001, 29), (1536, 2001, 28), (700, 1500, 4334)])
def test_long_lattice_strict_gate_at_modest_loss(dev, S, T, C):
    from lightning_asr_amd import ops
    g = torch.Generator().manual_seed(S + T)
    B = 3
    tl = torch.tensor([S, S - 61, S // 2], dtype=torch.int32)
    il = torch.tensor([T, T - 30, T // 2 + 5], dtype=torch.int32)
    tg = (torch.arange(S) % (C - 1)).repeat(B, 1)
    tg[:, 3] = tg[:, 2]                                                # one repeat (the even spacing leaves blanks between)
    for b in range(B):
        tg[b, int(tl[b]):] = 0
    lp = _peaked(B, T, C, tg, tl, il, g)
    gs = torch.rand(B, generator=g) + 0.5
    ref, gref, ok = _torch_ref(lp, tg, il, tl, gs)
    assert ok.all() and float(ref.max()) < 2e3, ref
    nll, grad = ops.ctc_loss(lp.to(dev), tg.to(dev), il.to(dev), tl.to(dev), C - 1, True, gs.to(dev))
    nll, grad = nll.cpu().double(), grad.cpu().double()
    assert ((nll - ref).abs() / ref.abs()).max() < 1e-4, (nll, ref)
    err_max, err_l2 = float((grad - gref).abs().max() / gref.abs().max()), rel_l2(grad, gref)
    assert err_max < 2e-3 and err_l2 < 2e-3, (err_max, err_l2, "torch f32:", _torch_f32_err(lp, tg, il, tl, gs, ok, gref))


def test_multi_wave_bit_identical_to_one_wave(dev):
    """labels of at most 500: width 500 takes the one-wave kernel (16 states per lane), widths 600 and 1500 the multi-wave kernels
    (2 and 3 waves): same per-state arithmetic, so any bit of difference would be the edge exchange"""
    from lightning_asr_amd import ops
    g = torch.Generator().manual_seed(9)
    B, T, C = 4, 1200, 28
    lp = F.log_softmax(torch.randn(B, T, C, generator=g) * 2, -1).to(dev)
    tl = torch.tensor([500, 480, 499, 250], dtype=torch.int32)
    il = torch.tensor([T, 1100, 1000, 700], dtype=torch.int32).to(dev)
    tg = _labels(B, 500, tl.tolist(), C, g, repeats=True)
    gs = torch.rand(B, generator=g).to(dev) + 0.5
    outs = []
    for W in (500, 600, 1500):
        tw = torch.zeros(B, W, dtype=torch.int64)
        tw[:, :500] = tg
        outs.append(ops.ctc_loss(lp, tw.to(dev), il, tl.to(dev), C - 1, True, gs))
    assert torch.isfinite(outs[0][0]).all()
    for nll, grad in outs[1:]:
        assert torch.equal(nll, outs[0][0])
        assert torch.equal(grad, outs[0][1])
    # and the register-ring form of both (C = 29: emission rows not in LDS)
    lp29 = F.log_softmax(torch.randn(B, 700, 29, generator=g), -1).to(dev)
    il29 = torch.tensor([700, 690, 680, 500], dtype=torch.int32).to(dev)
    r = []
    for W in (500, 1100):
        tw = torch.zeros(B, W, dtype=torch.int64)
        tw[:, :500] = tg
        r.append(ops.ctc_loss(lp29, tw.to(dev), il29, tl.to(dev), 28, True, gs))
    assert torch.equal(r[0][0], r[1][0]) and torch.equal(r[0][1], r[1][1])


@pytest.mark.parametrize("Cc,S", [(4334, 600), (4334, 2047), (5207, 2047)])
def test_lean_head_long_labels(dev, Cc, S):
    """lasr_gemm_rowstat + lasr_ctc_loss_lean (large-vocabulary head) with the multi-wave lattice against torch on the stored logits"""
    import ctypes as C
    from lightning_asr_amd import _lib
    from lightning_asr_amd._lib import call
    from lightning_asr_amd.ops import _p, _stream
    g = torch.Generator().manual_seed(Cc + S)
    B, K = 3, 64
    T = max(2 * S + 50, 1300)
    x = torch.randn(B * T, K, generator=g).bfloat16().float()
    W = (torch.randn(Cc, K, generator=g) * 0.3).bfloat16().float()
    bias = torch.randn(Cc, generator=g) * 0.1
    tl = torch.tensor([S, S - 100, 300], dtype=torch.int32)
    il = torch.tensor([T, T - 40, 900], dtype=torch.int32)
    tgt = _labels(B, S, tl.tolist(), Cc, g, repeats=True)
    ldc = (Cc + 7) // 8 * 8
    N = B * T
    logits = torch.empty(N, ldc, dtype=torch.bfloat16, device=dev)
    tiles = (Cc + 255) // 256
    rs = torch.empty(N * tiles * 2, dtype=torch.float32, device=dev)
    ra = torch.empty(N * tiles, dtype=torch.int32, device=dev)
    nt = C.c_int(0)
    xb, Wb, bias_d = x.to(dev, torch.bfloat16), W.to(dev, torch.bfloat16), bias.to(dev)
    tgt_d, il_d, tl_d = tgt.to(dev), il.to(dev), tl.to(dev)
    call("lasr_gemm_rowstat", _p(xb), _p(Wb), _p(bias_d), _p(logits), ldc, N, Cc, K, _p(rs), _p(ra), C.byref(nt), _stream())
    wsb = _lib.load().lasr_ctc_lean_workspace_bytes(B, T, Cc, S)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    am = torch.empty(N, dtype=torch.int32, device=dev)
    grad = torch.empty(N, ldc, dtype=torch.bfloat16, device=dev)
    db = torch.empty(Cc, dtype=torch.float32, device=dev)
    call("lasr_ctc_loss_lean", _p(logits), ldc, _p(rs), _p(ra), tiles, _p(tgt_d), _p(il_d), _p(tl_d), B, T, Cc, S,
         Cc - 1, _p(nll), _p(am), _p(grad), _p(db), None, _p(ws), wsb, _stream())
    torch.cuda.synchronize()
    got = logits[:, :Cc].float().cpu()
    lg = got.double().view(B, T, Cc).requires_grad_(True)
    lp = F.log_softmax(lg, -1)
    ref = F.ctc_loss(lp.transpose(0, 1), tgt, il.long(), tl.long(), blank=Cc - 1, reduction="none")
    assert torch.isfinite(ref).all()
    (ref.sum() / B).backward()
    assert ((nll.cpu().double() - ref.detach()).abs() / ref.detach().abs()).max() < 1e-4, (nll, ref)
    gg = grad[:, :Cc].float().cpu().view(B, T, Cc)
    # torch's own f32 CTC on the same logits: the yardstick of the gradient gate (see _check)
    lf = got.view(B, T, Cc).clone().requires_grad_(True)
    (F.ctc_loss(F.log_softmax(lf, -1).transpose(0, 1), tgt, il.long(), tl.long(), blank=Cc - 1, reduction="none").sum() / B).backward()
    for b in range(B):
        ref_b = lg.grad[b].float().bfloat16().float()
        e, ef = rel_l2(gg[b], ref_b), rel_l2(lf.grad[b].bfloat16().float(), ref_b)
        print("GATES lean", Cc, S, b, e, "torch f32:", ef)
        assert e < max(2e-3, 2 * ef), (b, e, ef)
        assert bool((gg[b, int(il[b]):] == 0).all())
    # decoder-bias gradient: column sums of the (unrounded) gradient
    ref_db = lg.grad.sum((0, 1))
    assert torch.isfinite(db).all()
    e, ef = rel_l2(db, ref_db), rel_l2(lf.grad.sum((0, 1)), ref_db)
    print("GATES lean bias", e, "torch f32:", ef)
    assert e < max(1e-3, 2 * ef), (e, ef)


def test_ctc_loss_rejects_labels_above_bound_before_launch(dev):
    from lightning_asr_amd import ops
    lp = torch.zeros(1, 8, 5, device=dev)
    with pytest.raises(ValueError, match="2047"):
        ops.ctc_loss(lp, torch.zeros(1, 2048, dtype=torch.int64, device=dev), torch.tensor([8], dtype=torch.int32, device=dev),
                     torch.tensor([1], dtype=torch.int32, device=dev), 4)


def _write_wav(path, secs, rng):
    L = int(secs * 16000)
    pcm = np.clip(0.1 * rng.standard_normal(L) * 32768, -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())


def test_trainer_validate_with_a_40s_clip(dev, tmp_path):
    """the reference validates clips up to 40 s (dev_max_duration: 40): a 600-character transcript of a 40 s clip (T' = 2001) in
    the dev manifest must validate, with val_loss = the mean of torch's CTC over the model's own log-probs"""
    import json
    from lightning_asr_amd.data_module import LibriDataModule
    from lightning_asr_amd.lightning_compat import Trainer, seed_everything
    from lightning_asr_amd.train import LightingModule
    labels = [c.strip() for c in open(os.path.join(ROOT, "data", "labels.txt"), encoding="utf-8").readlines()]
    rng = np.random.default_rng(4)
    man = tmp_path / "dev.json"
    with open(man, "w", encoding="utf-8") as mf:
        for i, (secs, S) in enumerate(((40.0, 600), (3.0, 8), (2.0, 5))):
            p = tmp_path / ("dev_%d.wav" % i)
            _write_wav(p, secs, rng)
            ids = rng.integers(0, len(labels), S)
            ids[1:6] = ids[0]                                          # repeats
            mf.write(json.dumps({"audio_filepath": str(p), "duration": secs, "text": "".join(labels[j] for j in ids)},
                                ensure_ascii=False) + "\n")
    seed_everything(0)
    dm = LibriDataModule([str(man)], str(man), str(man), labels, train_bs=4, dev_bs=4, num_worker=0, device=str(dev),
                         act_dtype=torch.float32)
    dm.setup()
    model = LightingModule(learning_rate=1e-2, weight_decay=1e-3, labels=labels, total_epoch=1, mask=True, use_cer=True, dtype="f32",
                           device=str(dev), warmup_steps=2)
    seen = []
    shared = model._shared

    def spy(batch):
        out, loss, t_lengths, trans, trans_lengths = shared(batch)
        seen.append((out.detach().cpu(), float(loss), t_lengths.cpu(), trans.cpu(), trans_lengths.cpu()))
        return out, loss, t_lengths, trans, trans_lengths
    model._shared = spy
    tr = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "run"), device=str(dev))
    model.trainer, tr.datamodule = tr, dm          # (as fit() attaches them: self.log records into the trainer)
    rec = tr.validate(model, dm)
    assert len(seen) == 1
    out, loss, tlen, trans, trl = seen[0]
    assert out.shape[1] == 2001 and trans.shape[1] == 600
    assert np.isfinite(rec["val_loss"]) and np.isfinite(loss)
    ref = F.ctc_loss(out.double().transpose(0, 1), trans.long(), tlen.long(), trl.long(), blank=len(labels), reduction="none")
    assert abs(rec["val_loss"] - float(ref.mean())) <= 1e-4 * abs(float(ref.mean())), (rec["val_loss"], ref)
    assert "val_wer_total" in rec and rec["val_wer_total"] >= 0
