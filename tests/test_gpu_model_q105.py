"""Whole-model parity of the "q105" variant (MyModel2 over the reference's QuartNet105: ten residual blocks of five separable
convolutions) on the native plan, f32: against the fixtures captured from the reference (tools/make_golden_q105.py) and against
the f64 helper oracle (tests/helpers/q105_oracle.py) on the same inputs; staged backward and graph replay against the plain step.

Gates.  Log-probs: noise = max |f32 helper oracle - f64 helper oracle| on the CPU, gate = max(2e-4, 4 noise) - 2e-4 is the plain
variant's gate (tests/test_gpu_model.py), the factor 4 covers a summation order that differs from the CPU's f32 order through 3.5
times as many BatchNorm layers.  Gradients: worst relative L2 over the tensors against the f64 oracle, gate = min(2e-2, max(6e-3,
2 r)) with r the same figure of the f32 CPU oracle against the f64 one (floor and cap of conftest.e2e_gate).  noise, r and the GPU's
errors are recorded through conftest.record_measured.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from oracle import ref_bf16 as E                       # noqa: E402
from oracle import ref_cpu as R                        # noqa: E402
from oracle.make_golden import checksum, golden_inputs  # noqa: E402
import q105_oracle as Q                                # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = {True: "tests/golden/model_q105.npz", False: "tests/golden/model_q105_nomask.npz"}
_CACHE = {}


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _native(dev, mask=True, dtype=torch.float32, n_class=28, gain=1.0):
    from lightning_asr_amd.engine import NativeModel
    m = NativeModel("q105", n_class, mask=mask, act="relu", dtype=dtype, device=dev)
    m.load_state_dict(Q.formula_state(n_class, gain=gain))
    return m


def _cpu_reference(key, mask, x, tg, pct, tsz, gain=1.0):
    """the helper oracle in f32 and in f64 on one batch, computed once per (batch, mask): forward (training and eval) log-probs,
    loss and gradients, running statistics after the training forward; and r, the f32 oracle's worst gradient distance from the f64 one"""
    if (key, mask) in _CACHE:
        return _CACHE[(key, mask)]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        o = Q.OracleModel(28, mask=mask, state=Q.cast_state(Q.formula_state(28, gain=gain), dt))
        o.training = False
        with torch.no_grad():
            lp_eval = o.forward(x.to(dt), pct).double()
        loss, nll, lp, grads = E.loss_and_grads(o, x.to(dt), tg, pct, tsz)
        out[tag] = {"lp_eval": lp_eval, "lp": lp.double(), "loss": loss, "nll": nll.double(), "grads": grads,
                    "state": {k: v.clone() for k, v in o.state.items()}}
    out["noise"] = float(max((out["f32"]["lp"] - out["f64"]["lp"]).abs().max(), (out["f32"]["lp_eval"] - out["f64"]["lp_eval"]).abs().max()))
    out["r"] = max(rel_l2(a, b) for a, b in zip(out["f32"]["grads"], out["f64"]["grads"]))
    _CACHE[(key, mask)] = out
    return out


def _grad_gate(r):
    return min(2e-2, max(6e-3, 2.0 * r))


def test_q105_state_dict_layout(dev):
    m = _native(dev)
    assert [(t.name, t.shape) for t in m.tensors] == [(k, tuple(s)) for k, s in Q.state_shapes(28)]
    assert len(m.tensors) == 425 and m.n_param == 11669340
    names = m.unit_names()
    assert len(names) == 52 and names[0] == "first_cnn" and names[-1] == "last_cnn2"
    assert names[1:6] == ["block1.seq.0", "block1.seq.1", "block1.seq.2", "block1.seq.3", "block1"]
    assert names[1:51] == [u[0] for u in Q.unit_table()]


@pytest.mark.parametrize("mask", [True, False])
def test_q105_forward_matches_golden_f32(dev, mask):
    from conftest import record_measured
    from lightning_asr_amd import ops
    gold = np.load(GOLD[mask])
    x, tg, pct, tsz = golden_inputs()
    ref = _cpu_reference("golden", mask, x, tg, pct, tsz, Q.GOLDEN_GAIN[mask])
    noise = ref["noise"]
    gate = max(2e-4, 4.0 * noise)
    tag = "q105_%s_golden_f32" % ("mask" if mask else "nomask")
    m = _native(dev, mask, gain=Q.GOLDEN_GAIN[mask])
    feats = ops.bct_to_btc(x[:, 0].contiguous().to(dev))
    lp_e, _ = m.forward(feats, pct.to(dev), training=False)
    err_e = float(np.abs(lp_e.cpu().numpy() - gold["eval_logprobs"]).max())
    lp, am = m.forward(feats, pct.to(dev), training=True)
    err = float(np.abs(lp.cpu().numpy() - gold["logprobs"]).max())
    print("%s: oracle f32-vs-f64 noise %.3e, gate %.3e, GPU eval err %.3e, training err %.3e" % (tag, noise, gate, err_e, err))
    record_measured(tag + "_oracle_noise", noise)
    record_measured(tag + "_logp_eval_abs_err", err_e)
    record_measured(tag + "_logp_abs_err", err)
    assert m.tap("lens").cpu().tolist() == gold["t_lengths"].tolist()
    assert err_e < gate, (err_e, gate)
    assert err < gate, (err, gate)
    # argmax (argmax_report's rule): a mismatch only where the reference's own top-1 / top-2 margin is below 2 noise, and at most
    # 1 % of the valid frames may be excused that way
    ref_lp = torch.from_numpy(gold["logprobs"]).double()
    top2 = ref_lp.topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    valid = torch.arange(margin.shape[1]).unsqueeze(0) < torch.from_numpy(gold["t_lengths"]).long().unsqueeze(1)
    mis = (am.cpu().long() != torch.from_numpy(gold["argmax"].astype("int64"))) & valid
    print("%s: %d of %d valid frames differ in argmax, margins there %s" % (tag, int(mis.sum()), int(valid.sum()), margin[mis].tolist()[:8]))
    assert bool((margin[mis] < 2.0 * noise).all()), (margin[mis].tolist(), noise)
    assert int(mis.sum()) <= 0.01 * int(valid.sum()), (int(mis.sum()), int(valid.sum()))
    for name in ["first_cnn", "block1", "block22", "block3", "block42", "block52", "last_cnn2"]:
        got = checksum(m.tap(name).transpose(1, 2).contiguous().cpu())
        assert np.abs(got - gold["tap_" + name]).max() < max(1e-4, gate), name
    # the suffix forms of lasr_model_tap for both kinds of unit name
    for name, c in (("block3.seq.0", 256), ("block3", 512)):
        assert tuple(m.tap(name + ".y").shape) == (4, 101, c) and tuple(m.tap(name + ".u").shape) == (4, 101, 256)
    assert tuple(m.tap("block3.y2").shape) == (4, 101, 512)
    with pytest.raises(KeyError):
        m.tap("block3.seq.0.y2")


def _check_loss_backward(dev, tag, mask, x, tg, pct, tsz, ref, gold=None, gain=1.0):
    from conftest import record_measured
    from lightning_asr_amd import ops
    m = _native(dev, mask, gain=gain)
    feats = ops.bct_to_btc(x[:, 0].contiguous().to(dev))
    loss, nll, lp, am = m.loss_backward(feats, pct.to(dev), tg.to(dev), tsz.to(dev))
    assert torch.isfinite(lp).all() and torch.isfinite(m.grads).all()
    nll_ref = torch.from_numpy(gold["nll"]).double() if gold is not None else ref["f64"]["nll"]
    loss_ref = float(gold["losses"][0]) if gold is not None else ref["f64"]["loss"]
    assert float((nll.cpu().double() - nll_ref).abs().max() / nll_ref.abs().max()) < 1e-4
    assert abs(loss.item() - loss_ref) / abs(loss_ref) < 1e-4
    if gold is not None:
        norms = np.array([m.view(t, m.grads).norm().item() for t in m.param_infos()])
        print("%s: grad norms vs the reference fixture, worst relative %.3e" % (tag, np.abs(norms / gold["grad_norms"] - 1).max()))
    rels = {t.name: rel_l2(m.view(t, m.grads), g) for t, g in zip(m.param_infos(), ref["f64"]["grads"])}
    worst = max(rels.values())
    gate = _grad_gate(ref["r"])
    print("%s: worst grad rel-L2 vs f64 oracle %.3e; f32 CPU oracle vs f64 r = %.3e; gate %.3e" % (tag, worst, ref["r"], gate))
    record_measured(tag + "_grad_rel_l2_vs_f64_oracle", worst)
    record_measured(tag + "_cpu_f32_oracle_grad_rel_l2_vs_f64_oracle", ref["r"])
    st = ref["f64"]["state"]
    for t in m.tensors:
        if t.kind == 1:
            assert rel_l2(m.view(t), st[t.name]) < 1e-4, t.name
    assert worst < gate, sorted(rels.items(), key=lambda kv: -kv[1])[:5]


@pytest.mark.parametrize("mask", [True, False])
def test_q105_loss_backward_matches_golden_f32(dev, mask):
    """nll, loss, running statistics and the gradients against the f64 helper oracle under min(2e-2, max(6e-3, 2 r)).

    The fixtures' weights are formula_state(gain = Q.GOLDEN_GAIN[mask]): the largest gain of 1, 0.7, 0.5, 0.35 at which the f32 CPU
    oracle itself is within 1e-2 of the f64 one (q105_oracle.GOLDEN_GAIN says why: with mask off and gain 1 ANY f32 evaluation of
    this model is 5e-2 from f64, r = 5.1e-2, the GPU 5.6e-2 - a fixture that cannot tell a right kernel from a wrong one).
    Measured on the MI355X:
      mask=True,  gain 1:    r = 4.9e-4, gate 6e-3,    GPU 3.1e-3.
      mask=False, gain 0.35: r = 5.2e-3, gate 1.03e-2, GPU 2.4e-3.
    At gain 1 the mask-off model's gradients are held PER UNIT (tests/test_gpu_units_q105.py::test_q105_units_b4_t101_nomask_f32)."""
    gold = np.load(GOLD[mask])
    x, tg, pct, tsz = golden_inputs()
    ref = _cpu_reference("golden", mask, x, tg, pct, tsz, Q.GOLDEN_GAIN[mask])
    _check_loss_backward(dev, "q105_%s_golden_f32" % ("mask" if mask else "nomask"), mask, x, tg, pct, tsz, ref, gold, Q.GOLDEN_GAIN[mask])


@pytest.mark.parametrize("B,lens", [(1, [17]), (4, [17, 1, 2, 3])], ids=["b1_t17", "b4_t17_masked_17_1_2_3"])
def test_q105_edge_shapes_f32(dev, B, lens):
    """T' = 17 (T_in = 33, one first_cnn window per output frame): every depthwise kernel from k = 39 up is wider than the sequence;
    with utterances masked down to 1, 2 and 3 frames the BatchNorm statistics run over mostly zero rows."""
    T_in, Tp, S = 33, 17, 3
    g = torch.Generator().manual_seed(B * 100 + T_in)
    x = torch.randn(B, 1, 64, T_in, generator=g)
    pct = torch.tensor([(n + 0.5) / Tp if n < Tp else 1.0 for n in lens], dtype=torch.float32)
    assert R.mask_lengths(Tp, pct).tolist() == lens
    x = x * (torch.arange(T_in).view(1, 1, 1, T_in) < (T_in * pct).int().view(B, 1, 1, 1))
    tg = torch.randint(0, 27, (B, S), generator=g)
    for b in range(B):
        for s in range(1, S):
            if tg[b, s] == tg[b, s - 1]:
                tg[b, s] = (tg[b, s] + 1) % 27
    tsz = torch.tensor([min(S, max(1, n // 2)) for n in lens], dtype=torch.int32)
    ref = _cpu_reference("edge_B%d" % B, True, x, tg, pct, tsz)
    _check_loss_backward(dev, "q105_edge_B%d_T33_f32" % B, True, x, tg, pct, tsz, ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_q105_staged_backward_equals_single_call(dev, dtype):
    """loss_backward_staged with 2 and 4 buckets and loss_backward_units (a stage per unit: a cut inside every block, so the residual
    gradient waits in the workspace across calls) give the gradients of loss_backward bit for bit; the announced ranges tile
    [0, n_param) exactly once."""
    from lightning_asr_amd import ops
    x, tg, pct, tsz = golden_inputs()
    feats = ops.bct_to_btc(x[:, 0].contiguous().to(dev), dtype)
    args = (feats, pct.to(dev), tg.to(dev), tsz.to(dev))
    m1 = _native(dev, True, dtype)
    m1.loss_backward(*args)
    torch.cuda.synchronize()
    assert torch.isfinite(m1.grads).all()
    for n_buckets in (2, 4):
        m2 = _native(dev, True, dtype)
        m2.grads.fill_(float("nan"))
        seen = []

        def on_bucket(ranges):
            torch.cuda.synchronize()
            for lo, hi in ranges:
                assert torch.isfinite(m2.grads[lo:hi]).all()          # final when announced
                seen.append((lo, hi))
        m2.loss_backward_staged(*args, on_bucket, n_buckets=n_buckets)
        torch.cuda.synchronize()
        assert len(seen) == n_buckets
        srt = sorted(seen)
        assert srt[0][0] == 0 and srt[-1][1] == m2.n_param and all(a[1] == b[0] for a, b in zip(srt[:-1], srt[1:])), seen
        assert torch.equal(m1.grads, m2.grads), n_buckets
    m3 = _native(dev, True, dtype)
    m3.grads.fill_(float("nan"))
    order = []
    m3.loss_backward_units(*args, lambda i, name: order.append(i))
    torch.cuda.synchronize()
    assert order == list(range(51, -1, -1))
    assert torch.equal(m1.grads, m3.grads)


def test_q105_graph_replay_equals_eager_bf16(dev):
    """two GraphedTrainStep replays against two eager TrainStep steps, B = 4, 32 000 samples (T_in = 201), bf16: bit for bit"""
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    B, L, S = 4, 32000, 12
    batches = []
    for s in range(2):
        wave, tg, tl = R.synth_batch(B, L, S, 27, seed=40 + s)
        batches.append((wave.to(dev), tg.to(dev), tl.to(dev)))

    def make():
        m = NativeModel("q105", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
        m.load_state_dict(Q.formula_state(28))
        return m, TrainStep(m, 1e-2, 1e-3)
    m0, ts0 = make()
    l0 = [float(ts0.step(w, tg, tl)[0].item()) for w, tg, tl in batches]
    m1, ts1 = make()
    g = GraphedTrainStep(ts1, B, L, S, prefetch=False, want_logp=True)
    g.capture(batches[0][0])
    l1 = [float(g.step(w, tg, tl)[0].item()) for w, tg, tl in batches]
    torch.cuda.synchronize()
    assert l0 == l1 and all(np.isfinite(l0))
    assert torch.equal(m0.params, m1.params) and torch.equal(m0.buffers, m1.buffers)


def test_q105_train_main_checkpoint_and_translate(dev, tmp_path):
    """`model.variant=q105` through train.main on a synthetic corpus - the fused Trainer.fit route with accumulation, EMA and norm
    clipping on - then the checkpoint through LightingModule.load_from_checkpoint and AsrTranslator (greedy and beam decoders)."""
    import json
    import subprocess
    data = tmp_path / "synth"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_data.py"), "--out", str(data), "--n-train", "8",
                    "--n-dev", "2", "--seconds", "2.0", "--ragged"], check=True)
    from lightning_asr_amd.train import LightingModule, main
    out = tmp_path / "run"
    tr = main(["data.train_manifest=[%s]" % (data / "train.json"), "data.val_manifest=%s" % (data / "dev.json"),
               "data.test_manifest=%s" % (data / "dev.json"), "data.labels=%s" % os.path.join(ROOT, "data", "labels.txt"),
               "model.variant=q105", "train.train_batch_size=2", "train.dev_batch_size=2", "train.total_epoch=1", "train.warmup_steps=1",
               "train.accumulate_grad_batches=2", "train.ema_decay=0.99", "train.gradient_clip_val=1.0",
               "train.gradient_clip_algorithm=norm", "output_dir=%s" % out])
    assert tr.global_step == 2
    rec = tr.history[-1]
    assert np.isfinite(rec["train_loss"]) and np.isfinite(rec["val_loss"]) and rec["train_loss"] > 0
    path = str(out / "checkpoints" / "last.ckpt")
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["hyper_parameters"]["variant"] == "q105"
    keys = [k for k in ckpt["state_dict"] if k.startswith("encoder.")]
    assert keys == ["encoder." + k for k, _ in Q.state_shapes(28)]
    m = LightingModule.load_from_checkpoint(path)
    m.eval()
    with torch.no_grad():
        lp = m(torch.zeros(1, 1, 64, 101, device=dev), torch.ones(1, device=dev))
    assert lp.shape == (1, 51, 28) and torch.isfinite(lp).all()
    from lightning_asr_amd.predict import AsrTranslator
    wav = json.loads(open(data / "dev.json").readline())["audio_filepath"]
    labels = ckpt["hyper_parameters"]["labels"]
    for kw in ({}, {"decoder": "beam", "beam_width": 4}):
        text = AsrTranslator(path, map_location="cuda", labels=labels, **kw).translate(wav)
        assert isinstance(text, str) and set(text) <= set(labels)
