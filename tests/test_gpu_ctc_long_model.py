"""Long transcripts through the model: the reference's dev shape (a 40 s clip, T' = 2001) against the f64 oracle, one training step at
S_max = 700 against the oracle, and the large-vocabulary head's lasr_model_loss_backward at S_max = 600 / 2047 (with and without the
feature prefetch riding in the step)."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _targets(B, S_max, lens, V, g):
    tg = torch.randint(0, V, (B, S_max), generator=g)
    tg[:, 1::7] = tg[:, 0::7][:, :tg[:, 1::7].shape[1]]          # adjacent repeats
    for b in range(B):
        tg[b, lens[b]:] = 0
    return tg


def test_dev_shape_40s_clip_matches_oracle(dev):
    """B = 2: one 40 s clip (L = 640 000 -> T_in = 4001, T' = 2001) with 600 labels and one 12 s clip with 150, f32, all three
    variants: mel, eval log-probs, per-sample nll, argmax, greedy collapse and CER against the f64 oracle"""
    from lightning_asr_amd import ops
    from lightning_asr_amd.engine import NativeModel
    g = torch.Generator().manual_seed(40)
    Ls = [640000, 192000]
    wave = 0.1 * torch.randn(2, Ls[0], generator=g)
    wave[1, Ls[1]:] = 0
    # mel of each clip at its own length (the 40 s one at L = 640 000) against the oracle in f64
    feats, frames = [], []
    for b in range(2):
        got = ops.mel(wave[b:b + 1, :Ls[b]].to(dev), None, None, None, True, torch.float32)[0][0].cpu().double()
        ref = R.parse_wave(wave[b:b + 1, :Ls[b]].double())[0]
        assert got.shape == ref.shape
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err < 1e-4, ("mel", Ls[b], err)
        feats.append(ref)
        frames.append(ref.shape[1])
    T_in = frames[0]
    assert T_in == 4001
    x = torch.zeros(2, 1, 64, T_in, dtype=torch.float64)
    x[0, 0] = feats[0]
    x[1, 0, :, :frames[1]] = feats[1]
    pct = torch.tensor([1.0, frames[1] / T_in], dtype=torch.float32)
    tl = torch.tensor([600, 150], dtype=torch.int32)
    tg = _targets(2, 600, tl.tolist(), 27, g)
    for variant in ("plain", "context", "context_se"):
        st64 = {k: (v.double() if v.is_floating_point() else v) for k, v in R.formula_state(variant, 28).items()}
        om = R.OracleModel(variant, 28, mask=True, state=st64)
        om.training = False
        with torch.no_grad():
            lp_ref = om.forward(x, pct)
        m = NativeModel(variant, 28, mask=True, act="relu", dtype=torch.float32, device=dev)
        m.load_state_dict(R.formula_state(variant, 28))
        lp, am = m.forward(ops.bct_to_btc(x[:, 0].float().contiguous().to(dev)), pct.to(dev), training=False)
        lp, am = lp.cpu().double(), am.cpu().long()
        assert lp.shape[1] == 2001
        t_len = R.mask_lengths(lp.shape[1], pct)
        valid = torch.arange(lp.shape[1]).view(1, -1) < t_len.view(-1, 1)
        lerr = float((lp - lp_ref).abs()[valid].max())
        assert lerr < 2e-3, (variant, lerr)
        # per-sample nll of the kernels' loss on the kernels' log-probs against the oracle's CTC on its own log-probs
        nll, _ = ops.ctc_loss(lp.float().to(dev), tg.to(dev), t_len.to(dev, torch.int32), tl.to(dev), 27, False)
        nll_ref = R.ctc_loss_per_sample(lp_ref, tg, t_len, tl, 27)
        nrel = float(((nll.cpu().double() - nll_ref).abs() / nll_ref.abs()).max())
        assert nrel < 1e-4, (variant, nll, nll_ref)
        # argmax: every frame that differs must be a near-tie of the oracle (top-1 / top-2 margin within twice the log-prob error)
        am_ref = lp_ref.argmax(-1)
        top2 = lp_ref.topk(2, -1).values
        margin = top2[..., 0] - top2[..., 1]
        bad = (am != am_ref) & valid
        report = [(int(b), int(t), float(margin[b, t])) for b, t in bad.nonzero().tolist()]
        assert all(mg <= 2 * lerr for _, _, mg in report), (variant, len(report), report[:20])
        # greedy collapse and CER: the device decode of the kernels' argmax against the oracle's decode of the same argmax
        tok, n = ops.greedy_decode(am.to(dev, torch.int32), t_len.to(dev, torch.int32), 27)
        dist, units = ops.edit_distance_batch(tok, n, tg.to(dev), tl.to(dev))
        tok, n, dist = tok.cpu(), n.cpu(), dist.cpu()
        for b in range(2):
            ref_tokens = R.greedy_collapse(am[b, :int(t_len[b])].tolist(), 27)
            assert tok[b, :int(n[b])].tolist() == ref_tokens
            assert int(dist[b]) == R.levenshtein(ref_tokens, tg[b, :int(tl[b])].tolist())
            assert int(units[b]) == int(tl[b])


def test_train_step_long_labels_matches_oracle(dev):
    """one TrainStep in f32 (plain, two 30 s clips, S_max = 700) against the oracle's training step"""
    from conftest import e2e_gate
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.step import TrainStep
    g = torch.Generator().manual_seed(30)
    B, L = 2, 480000
    wave = 0.1 * torch.randn(B, L, generator=g)
    tl = torch.tensor([700, 520], dtype=torch.int32)
    tg = _targets(B, 700, tl.tolist(), 27, g)
    feats = torch.stack([R.parse_wave(wave[i:i + 1].double())[0] for i in range(B)]).unsqueeze(1)
    st64 = {k: (v.double() if v.is_floating_point() else v) for k, v in R.formula_state("plain", 28).items()}
    om = R.OracleModel("plain", 28, mask=True, state=st64)
    st = R.NovogradState(len(om.parameters()))
    loss_ref, grads_ref = R.train_step(om, st, feats, tg, torch.ones(B), tl, 1e-2, 1e-3)
    m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.float32, device=dev)
    m.load_state_dict(R.formula_state("plain", 28))
    ts = TrainStep(m, 1e-2, 1e-3)
    loss, nll, logp, am = ts.step(wave.to(dev), tg.to(dev), tl.to(dev))
    torch.cuda.synchronize()
    assert logp.shape[1] == 1501
    assert abs(loss.item() - loss_ref) / abs(loss_ref) < 1e-4, (loss.item(), loss_ref)
    rels = {t.name: rel_l2(m.view(t, m.grads), gr) for t, gr in zip(m.param_infos(), grads_ref)}
    worst = max(rels.values())
    print("train step long labels: worst grad rel L2 vs f64 oracle", worst)
    assert worst < e2e_gate("long_labels_train_step_f32_grad_rel_l2_vs_f64_oracle"), sorted(rels.items(), key=lambda kv: -kv[1])[:5]


@pytest.mark.parametrize("S", [600, 2047])
def test_lean_head_model_loss_backward_long_labels(dev, S):
    """lasr_model_loss_backward on the large-vocabulary head (bf16, C = 4334) with S_max > 511: per-sample nll and the bf16 logit
    gradient against torch on the stored logits, the decoder-bias gradient against torch's and against the dense head's, and the
    same bits with the next batch's features computed in the step (set_prefetch)"""
    from lightning_asr_amd import ops
    from lightning_asr_amd.engine import NativeModel
    C = 4334
    g = torch.Generator().manual_seed(S)
    L = int(16000 * (1.3 * S / 50 + 1))                         # T' ~ 1.3 S + 50 frames: feasible with the repeats
    B = 2
    wave = (0.1 * torch.randn(B, L, generator=g)).to(dev)
    nxt = (0.1 * torch.randn(B, 48000, generator=g)).to(dev)
    tl = torch.tensor([S, S - 90], dtype=torch.int32)
    tg = _targets(B, S, tl.tolist(), C - 1, g)
    res = []
    for prefetch in (False, True):
        m = NativeModel("plain", C, mask=True, dtype=torch.bfloat16, device=dev)
        m.init_parameters(4)
        assert m.lean_head
        _, feats, _, pct = ops.mel(wave, None, None, None, True, torch.bfloat16, want_bft=False)
        nf = None
        if prefetch:
            nf, npct = m.arm_prefetch(nxt)
        loss, nll, logp, am = m.loss_backward(feats, pct, tg.to(dev), tl.to(dev), want_logp=False)
        assert logp is None
        if not prefetch:
            _, nf, _, npct = ops.mel(nxt, None, None, None, True, torch.bfloat16, want_bft=False)
        torch.cuda.synchronize()
        bias_t = [t for t in m.param_infos() if t.name == "decoder.bias"][0]
        res.append((loss.clone(), nll.clone(), m.grads.clone(), nf.clone(), npct.clone(), am.clone()))
        if not prefetch:
            T = m.out_frames(feats.shape[1])
            assert T >= S + 200
            logits = m.tap("logits_bf16")[:, :, :C].float().cpu()
            glog = m.tap("grad_logits_bf16")[:, :, :C].float().cpu()
            db = m.view(bias_t, m.grads).detach().cpu().double()
            t_len = ops.mask_lengths(pct, T).cpu()
            lg = logits.double().requires_grad_(True)
            ref = F.ctc_loss(F.log_softmax(lg, -1).transpose(0, 1), tg, t_len.long(), tl.long(), blank=C - 1, reduction="none")
            (ref.sum() / B).backward()
            lf = logits.clone().requires_grad_(True)
            (F.ctc_loss(F.log_softmax(lf, -1).transpose(0, 1), tg, t_len.long(), tl.long(), blank=C - 1, reduction="none").sum()
             / B).backward()
            assert ((nll.cpu().double() - ref.detach()).abs() / ref.detach().abs()).max() < 1e-4, (nll, ref)
            for b in range(B):
                e, ef = rel_l2(glog[b], lg.grad[b].float().bfloat16()), rel_l2(lf.grad[b].bfloat16(), lg.grad[b].float().bfloat16())
                assert e < max(2e-3, 2 * ef), (b, e, ef)
            ref_db = lg.grad.sum((0, 1))
            e, ef = rel_l2(db, ref_db), rel_l2(lf.grad.sum((0, 1)), ref_db)
            assert torch.isfinite(db).all() and e < max(1e-3, 2 * ef), (e, ef)
            # the dense head of the same model (f32 log-probs from the unrounded logits): the same gradient up to the bf16
            # rounding of the logits the lean head reads
            m.loss_backward(feats, pct, tg.to(dev), tl.to(dev), want_logp=True)
            torch.cuda.synchronize()
            db_dense = m.view(bias_t, m.grads).detach().cpu().double()
            ed = rel_l2(db, db_dense)
            print("lean vs dense bias gradient rel L2", S, ed, "lean vs torch", e, "torch f32", ef)
            assert ed < 2e-2, ed
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert torch.isfinite(res[0][0]).all()
