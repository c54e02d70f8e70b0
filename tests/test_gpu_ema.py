"""GPU tier of the weight EMA ("Weight EMA"): the standalone kernel bit for bit against torch's three eager operations, the
update fused into the optimiser step bit for bit against step + standalone kernel, the drift against an f64 recurrence, the
training step (plain, accumulating, graph-replayed), NativeModel.using_params, Trainer.fit on both routes with its checkpoints and
resume, and the weights AsrTranslator picks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
LABELS = [c.strip() for c in open(os.path.join(ROOT, "data", "labels.txt")).readlines()]
B, L, S = 2, 16000, 5              # T_in = 101, as tests/test_gpu_grad_accum.py


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- 1. the standalone kernel ----------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 255, 256, 257, 16389, 70001)
WEIGHTS = (0.0, 2.0 ** -14, float(np.float32(0.1)), 0.5, 1.0)


@pytest.mark.parametrize("off_e, off_p", [(0, 0), (1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("n", SIZES)
def test_ema_kernel_is_the_torch_expression_bit_for_bit(dev, n, off_e, off_p):
    """both buffers aligned, both sliced as flat[1:], and one only; the bytes around the slice and ``params`` stay as they were"""
    from lightning_asr_amd import ops
    g = torch.Generator().manual_seed(1000 + n)
    pad = 5
    for w in WEIGHTS:
        flat_e = torch.randn(n + off_e + pad, generator=g).to(dev)
        flat_p = (torch.randn(n + off_p + pad, generator=g) * 3).to(dev)
        e, p = flat_e[off_e:off_e + n], flat_p[off_p:off_p + n]
        want = e + (p - e) * w                       # three eager f32 operations, one rounding each
        e0, p0 = flat_e.clone(), flat_p.clone()
        ops.ema_update(e, p, w)
        torch.cuda.synchronize()
        assert _same_bits(e, want), (n, w, float((e - want).abs().max()))
        assert _same_bits(flat_p, p0)
        assert _same_bits(flat_e[:off_e], e0[:off_e]) and _same_bits(flat_e[off_e + n:], e0[off_e + n:])


def test_ema_kernel_signed_zeros_denormals_and_arguments(dev):
    from lightning_asr_amd import _lib, ops
    tiny = 2.0 ** -140                                 # an f32 denormal
    vals = [0.0, -0.0, tiny, -tiny, 3 * tiny, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0, 1e-30, 1e38]       # (no pair overflows: a NaN's payload is not compared)
    e = torch.tensor([a for a in vals for _ in vals], dtype=torch.float32, device=dev)
    p = torch.tensor([b for _ in vals for b in vals], dtype=torch.float32, device=dev)
    for w in WEIGHTS:
        got = e.clone()
        want = e + (p - e) * w
        ops.ema_update(got, p, w)
        torch.cuda.synchronize()
        assert _same_bits(got, want), w
    # refusals of the wrapper: dtype, shape, device; an empty pair is a no-op
    ops.ema_update(e[:0], p[:0], 0.5)
    with pytest.raises(TypeError):
        ops.ema_update(e.double(), p.double(), 0.5)
    with pytest.raises(ValueError):
        ops.ema_update(e, p[:-1], 0.5)
    with pytest.raises(ValueError):
        ops.ema_update(e.view(11, 11), p.view(11, 11), 0.5)
    with pytest.raises(_lib.LasrError):
        ops.ema_update(e, p.cpu(), 0.5)
    with pytest.raises(_lib.LasrError):
        ops.ema_update(e, e, 0.5)                       # aliasing: LASR_E_ARG from the library
    st = ops.ema_state(0.5, device=dev)
    with pytest.raises(ValueError):
        ops.novograd_step(p, p, p, p[:1], torch.zeros(2, dtype=torch.int64, device=dev), p[:1], ema=e)          # no state
    with pytest.raises(ValueError):
        ops.novograd_step(p, p, p, p[:1], torch.zeros(2, dtype=torch.int64, device=dev), p[:1], ema_state=st)   # no ema


# ---- 2. / 3. fused into the optimiser step ---------------------------------------------------------------------------------------
STEPS, DECAY = 12, 0.5
_RUNS = {}


def _offsets(n):
    return [0, 1, 4, 9, 16, 21, 1045, n]               # tensor boundaries off multiples of 4: the scalar path runs too


def _fused_run(dev, n, keep):
    """12 optimiser steps on a hand-made tensor table, twice from one start: path A with the EMA inside novograd_step, path B the
    step without it followed by the standalone kernel with the host twin's weight.  Computed once per (n, keep) and left alone."""
    key = (n, keep)
    if key in _RUNS:
        return _RUNS[key]
    from lightning_asr_amd import ops
    g = torch.Generator().manual_seed(77 + n)
    offs = torch.tensor(_offsets(n), dtype=torch.int64, device=dev)
    n_t = offs.numel() - 1
    p0 = torch.randn(n, generator=g).to(dev)
    grads = [(torch.randn(n, generator=g) * (0.1 + k)).to(dev) for k in range(STEPS)]
    lr = torch.tensor([1e-2], dtype=torch.float32, device=dev)

    def start():
        return {"p": p0.clone(), "m": torch.zeros_like(p0), "v": torch.zeros(n_t, dtype=torch.float32, device=dev), "e": p0.clone(),
                "ws": ops.novograd_workspace(n_t, n, dev) if keep else None}
    a, b = start(), start()
    st = ops.ema_state(DECAY, True, 0, device=dev)
    trace, same, weights = [], [], []
    for k in range(STEPS):
        ops.novograd_step(a["p"], grads[k], a["m"], a["v"], offs, lr, 0.8, 0.5, 1e-8, 1e-3, ws=a["ws"], ema=a["e"], ema_state=st)
        ops.novograd_step(b["p"], grads[k], b["m"], b["v"], offs, lr, 0.8, 0.5, 1e-8, 1e-3, ws=b["ws"])
        w = ops.ema_weight(DECAY, True, k)
        ops.ema_update(b["e"], b["p"], w)
        torch.cuda.synchronize()
        same.append({x: _same_bits(a[x], b[x]) for x in ("p", "m", "v", "e")})
        weights.append(float(w))
        trace.append((a["p"].cpu().numpy().copy(), a["e"].cpu().numpy().copy()))
    _RUNS[key] = {"same": same, "state": ops.ema_state_read(st), "weights": weights, "trace": trace, "p0": p0.cpu().numpy().copy()}
    return _RUNS[key]


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("n", [1046, 16389, 70001])
def test_fused_ema_equals_step_then_kernel_bit_for_bit(dev, n, keep):
    from lightning_asr_amd import ops
    run = _fused_run(dev, n, keep)
    for k, s in enumerate(run["same"]):
        assert all(s.values()), (k, s)
    assert run["state"]["num_updates"] == STEPS
    assert run["state"]["w"] == float(ops.ema_weight(DECAY, True, STEPS - 1)) == 0.5
    assert run["state"]["decay"] == DECAY and run["state"]["warmup"] is True
    assert run["weights"][7] > 0.5 and run["weights"][8] == 0.5          # the ramp crossed the cap at t = 8
    e_first = run["trace"][0][1]
    assert not np.array_equal(e_first, run["p0"])                        # the average moved at all


@pytest.mark.parametrize("keep", [False, True])
def test_new_entry_without_ema_is_the_old_entry_bit_for_bit(dev, keep):
    from lightning_asr_amd import _lib, ops
    from lightning_asr_amd.ops import _p, _stream
    n = 16389
    g = torch.Generator().manual_seed(5)
    offs = torch.tensor(_offsets(n), dtype=torch.int64, device=dev)
    n_t = offs.numel() - 1
    p0 = torch.randn(n, generator=g).to(dev)
    lr = torch.tensor([1e-2], dtype=torch.float32, device=dev)
    a = {"p": p0.clone(), "m": torch.zeros_like(p0), "v": torch.zeros(n_t, dtype=torch.float32, device=dev)}
    b = {k: v.clone() for k, v in a.items()}
    ws_a, ws_b = ops.novograd_workspace(n_t, n, dev), ops.novograd_workspace(n_t, n, dev)
    for k in range(3):
        gr = torch.randn(n, generator=g).to(dev)
        ops.novograd_step(a["p"], gr, a["m"], a["v"], offs, lr, 0.8, 0.5, 1e-8, 1e-3, grad_scale=0.5, ws=ws_a if keep else None)
        if not keep:
            ws_b.random_(0, 255)                       # a workspace the caller does not keep may hold anything
        _lib.call("lasr_novograd_step_ema", _p(b["p"]), _p(gr), _p(b["m"]), _p(b["v"]), _p(offs), n_t, n, _p(lr), 0.8, 0.5, 1e-8, 1e-3,
                  0.5, _p(ws_b), ws_b.numel(), _stream(), None, None, int(keep))
        torch.cuda.synchronize()
        for x in a:
            assert _same_bits(a[x], b[x]), (k, x)


def test_fused_ema_drift_against_f64(dev):
    """the f64 recurrence fed the GPU's own parameter sequence and the device's own f32 weights: what is left is the rounding of
    the update, bounded per element by 5 * 2^-24 * M / (1 - d_max) (derivation: tests/helpers/ema_oracle.py)"""
    import ema_oracle
    run = _fused_run(dev, 70001, True)
    params = [p for p, _ in run["trace"]]
    _, oracle = ema_oracle.recurrence(run["p0"], params, run["weights"])
    M = max(max(float(np.abs(p).max()), float(np.abs(e).max())) for p, e in run["trace"])
    M = max(M, float(np.abs(run["p0"]).max()))
    d_max = max(1.0 - w for w in run["weights"])
    assert d_max == DECAY
    bound = ema_oracle.drift_bound(M, d_max)
    for k, ((_, e_gpu), e64) in enumerate(zip(run["trace"], oracle)):
        err = float(np.abs(e_gpu.astype(np.float64) - e64).max())
        print("step %d: max |e_gpu - e_f64| = %.3e (bound %.3e)" % (k, err, bound))
        assert err <= bound, (k, err, bound)


# ---- 4. the training step ---------------------------------------------------------------------------------------------------
def _model(dev, dtype=torch.float32, seed=5):
    from lightning_asr_amd.engine import NativeModel
    m = NativeModel("plain", 28, mask=True, act="relu", dtype=dtype, device=dev)
    m.init_parameters(seed=seed)
    return m


def _schedule():
    from lightning_asr_amd.schedule import CosineAnnealingWarmupRestarts
    return CosineAnnealingWarmupRestarts(None, first_cycle_steps=100, cycle_mult=2, max_lr=1e-2, min_lr=1e-4, warmup_steps=3, gamma=0.5)


@pytest.fixture(scope="module")
def batches(dev):
    out = []
    for s in range(4):
        wave, tg, tl = R.synth_batch(B, L, S, 27, seed=700 + s)
        out.append((wave.to(dev), tg.to(dev), tl.to(dev)))
    return out


def test_trainstep_ema_follows_the_recurrence_and_leaves_training_alone(dev, batches):
    from lightning_asr_amd import ops
    from lightning_asr_amd.step import TrainStep
    m0, m1 = _model(dev), _model(dev)
    ts0 = TrainStep(m0, 1e-2, 1e-3, schedule=_schedule())
    ts1 = TrainStep(m1, 1e-2, 1e-3, schedule=_schedule(), ema_decay=0.9)
    assert ts0.ema is None and ts0.ema_state is None and ts0.ema_num_updates == 0
    assert _same_bits(ts1.ema, m1.params) and ts1.ema.data_ptr() != m1.params.data_ptr()
    hand = m1.params.clone()
    for k in range(3):
        l0 = ts0.step(*batches[k])[0]
        l1 = ts1.step(*batches[k])[0]
        hand = hand + (m1.params - hand) * float(ops.ema_weight(0.9, True, k))
        torch.cuda.synchronize()
        assert _same_bits(l0, l1)
        assert _same_bits(m0.params, m1.params) and _same_bits(m0.buffers, m1.buffers), k      # the average does not perturb training
        assert _same_bits(ts0.exp_avg, ts1.exp_avg) and _same_bits(ts0.exp_avg_sq, ts1.exp_avg_sq)
        assert _same_bits(ts1.ema, hand), (k, float((ts1.ema - hand).abs().max()))
    assert ts1.ema_num_updates == 3
    assert not _same_bits(ts1.ema, m1.params)


def test_accumulating_trainstep_updates_the_ema_on_boundaries_only(dev, batches):
    from lightning_asr_amd import ops
    from lightning_asr_amd.step import TrainStep
    m = _model(dev)
    ts = TrainStep(m, 1e-2, 1e-3, schedule=_schedule(), accumulate=2, ema_decay=0.9)
    counts = []
    for k in range(4):
        before, p_before = ts.ema.clone(), m.params.clone()
        ts.step(*batches[k])
        torch.cuda.synchronize()
        counts.append(ts.ema_num_updates)
        if k % 2 == 0:                          # an accumulate micro-step: neither the parameters nor the average move
            assert _same_bits(ts.ema, before) and _same_bits(m.params, p_before)
        else:
            want = before + (m.params - before) * float(ops.ema_weight(0.9, True, k // 2))
            assert not _same_bits(ts.ema, before) and _same_bits(ts.ema, want)
    assert counts == [0, 1, 1, 2] and ts.global_step == 2


# ---- 5. graph ----------------------------------------------------------------------------------------------------------------
def test_graph_replays_the_ema_and_its_warmup(dev, batches):
    from lightning_asr_amd import ops
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep

    def make():
        m = _model(dev, torch.bfloat16, seed=9)
        ts = TrainStep(m, 1e-2, 1e-3, schedule=_schedule(), ema_decay=0.9)
        ts.use_device_schedule()
        return m, ts
    m0, ts0 = make()
    m1, ts1 = make()
    ts0.step(*batches[3])                        # one eager step on both first: the capture starts from an average that differs
    ts1.step(*batches[3])                        # from the parameters and from a count of 1
    before = {"ema": ts1.ema.clone(), "state": ts1.ema_state.clone(), "params": m1.params.clone()}
    g = GraphedTrainStep(ts1, B, L, S, prefetch=False, want_logp=True)
    g.capture(batches[0][0])
    assert _same_bits(ts1.ema, before["ema"]) and torch.equal(ts1.ema_state, before["state"]) and _same_bits(m1.params, before["params"])
    assert ts1.ema_num_updates == 1
    for k in range(3):
        w, tg, tl = batches[k]
        l0 = ts0.step(w, tg, tl)[0]
        l1 = g.step(w, tg, tl)[0]
        torch.cuda.synchronize()
        assert _same_bits(l0, l1)
        assert _same_bits(m0.params, m1.params) and _same_bits(ts0.ema, ts1.ema), k
        s0, s1 = ops.ema_state_read(ts0.ema_state), ops.ema_state_read(ts1.ema_state)
        assert s0 == s1 and s1["num_updates"] == k + 2
        assert s1["w"] == float(ops.ema_weight(0.9, True, k + 1))             # the weight follows the ramp across replays
    assert ts1.global_step == 4


# ---- 6. using_params ---------------------------------------------------------------------------------------------------------
def test_using_params_swaps_without_copying(dev, batches):
    from lightning_asr_amd import ops
    m, m2 = _model(dev), _model(dev, seed=6)
    ema = m.params + 0.01 * torch.randn(m.n_param, generator=torch.Generator().manual_seed(3)).to(dev)
    m2.params.copy_(ema)
    m2.buffers.copy_(m.buffers)
    _, feats, _, pct = ops.mel(batches[0][0], None, None, None, True, torch.float32, want_bft=False, want_btf=True)
    live = m.params
    ptr, snapshot = m.params.data_ptr(), m.params.clone()
    base = m.forward(feats, pct, training=False)[0].clone()
    with m.using_params(ema) as mm:
        assert mm is m and m.params is ema
        got = m.forward(feats, pct, training=False)[0].clone()
    want = m2.forward(feats, pct, training=False)[0]
    torch.cuda.synchronize()
    assert _same_bits(got, want) and not _same_bits(got, base)
    assert m.params is live and m.params.data_ptr() == ptr and _same_bits(m.params, snapshot)
    with pytest.raises(RuntimeError, match="inside"):
        with m.using_params(ema):
            raise RuntimeError("inside")
    assert m.params is live and m.params.data_ptr() == ptr
    assert _same_bits(m.forward(feats, pct, training=False)[0], base)
    for bad in (ema[:-1], ema.double(), ema.cpu(), ema.view(1, -1)):
        with pytest.raises(ValueError):
            with m.using_params(bad):
                pass
    assert m.params is live


# ---- 7. Trainer.fit, both routes ----------------------------------------------------------------------------------------------
def _kw(dtype):
    return dict(learning_rate=1e-2, weight_decay=1e-3, labels=LABELS, total_epoch=1, drop_rate=0.0, mask=True, use_cer=True, dtype=dtype,
                warmup_steps=2)


def _act(dtype):
    return torch.float32 if dtype == "f32" else torch.bfloat16


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    data = tmp_path_factory.mktemp("ema") / "synth"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_data.py"), "--out", str(data), "--n-train", "32",
                    "--n-dev", "4", "--seconds", "2.0"], check=True)
    return data


def _datamodule(data, dev, dtype):
    from lightning_asr_amd.data_module import LibriDataModule
    return LibriDataModule([str(data / "train.json")], str(data / "dev.json"), str(data / "dev.json"), LABELS, train_bs=4, dev_bs=4,
                           num_worker=2, device=str(dev), act_dtype=_act(dtype), train_crop=False)


def _fit(dev, corpus, root, dtype, cls=None, n_batches=8, **trainer_kw):
    from lightning_asr_amd.lightning_compat import Trainer, seed_everything
    from lightning_asr_amd.train import LightingModule
    seed_everything(0)
    dm = _datamodule(corpus, dev, dtype)
    model = (cls or LightingModule)(device=str(dev), **_kw(dtype))
    tr = Trainer(max_epochs=1, default_root_dir=str(root), device=str(dev), check_val_every_n_epoch=1, limit_train_batches=n_batches,
                 **trainer_kw)
    tr.fit(model, dm)
    torch.cuda.synchronize()
    return tr, model, dm


def _validate_loaded(dev, corpus, state_dict, dtype):
    """val_loss of a fresh module holding `state_dict`, validated by a fresh Trainer (no optimiser, so no average: its live
    parameters are what it reads) on the same dev set: the same files, the same features"""
    from lightning_asr_amd.lightning_compat import Trainer
    from lightning_asr_amd.train import LightingModule
    model = LightingModule(device=str(dev), **_kw(dtype))
    model.load_state_dict(state_dict)
    tr = Trainer(device=str(dev))
    dm = _datamodule(corpus, dev, dtype)
    model.trainer = tr
    dm.trainer = tr
    dm.setup("fit")
    return tr.validate(model, dm)["val_loss"]


def _check_ema_fit(dev, corpus, tr, model, steps, dtype):
    from lightning_asr_amd.lightning_compat import Trainer
    from lightning_asr_amd.train import LightingModule
    opt, native = tr._opt, model.encoder.native
    assert tr.global_step == steps and opt.ema is not None and opt.ema_num_updates == steps
    ckpt_path = os.path.join(tr.root, "checkpoints", "last.ckpt")
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
    sd, esd = ckpt["state_dict"], ckpt["ema_state_dict"]
    assert list(sd.keys()) == list(esd.keys())
    assert ckpt["ema"] == {"decay": 0.9, "warmup": True, "num_updates": steps} and ckpt["global_step"] == steps
    param_keys = {"encoder." + t.name for t in native.param_infos()}
    for t in native.tensors:
        key = "encoder." + t.name
        if key in param_keys:
            assert _same_bits(esd[key], native.view(t, opt.ema).cpu()), key
            assert _same_bits(sd[key], native.view(t).cpu()), key                   # state_dict stays the live weights
        else:
            assert torch.equal(esd[key], sd[key]), key                              # buffers: the live ones
    assert any(not torch.equal(esd[k], sd[k]) for k in param_keys)
    # ema_eval: the recorded val_loss belongs to the averaged model, not to the live one
    recorded = tr.history[-1]["val_loss"]
    v_ema, v_live = _validate_loaded(dev, corpus, esd, dtype), _validate_loaded(dev, corpus, sd, dtype)
    print("val_loss recorded %.9g, from ema_state_dict %.9g, from state_dict %.9g" % (recorded, v_ema, v_live))
    # Two module instances run the same eval forward on workspaces laid out for different histories (the fitted one has trained,
    # the loaded one has not), and the f32 kernels' summation order may follow the layout: the two f32 losses agree to a few
    # units of f32 resolution (2^-23 relative), not always in every bit.  8 units are allowed; the live model's loss is some
    # thousand units away, which is what the check has to tell apart.
    ulp = 2.0 ** -23 * abs(recorded)
    assert abs(recorded - v_ema) <= 8 * ulp, (recorded, v_ema)
    assert abs(recorded - v_live) > 1000 * ulp, (recorded, v_live)
    # resume: the average and its count come back through the optimiser state, before the first step
    model2 = LightingModule(device=str(dev), **_kw(dtype))
    tr2 = Trainer(max_epochs=1, default_root_dir=os.path.join(tr.root, "resumed"), device=str(dev), ema_decay=0.9,
                  resume_from_checkpoint=ckpt_path)
    tr2.fit(model2, _datamodule(corpus, dev, dtype))                                       # epoch 0 is done: nothing is trained
    assert tr2.global_step == steps and tr2._opt is not opt
    saved = ckpt["optimizer_states"][0]["lasr"]
    assert saved["ema_num_updates"] == steps and saved["ema_decay"] == 0.9 and saved["ema_warmup"] is True
    assert _same_bits(tr2._opt.ema.cpu(), saved["ema"]) and _same_bits(tr2._opt.ema, opt.ema)
    assert tr2._opt.ema_num_updates == steps
    assert _same_bits(model2.encoder.native.params, native.params)
    return ckpt_path


@pytest.fixture(scope="module")
def fused_fit(dev, corpus, tmp_path_factory):
    old = os.environ.get("LASR_TRAINER_GRAPH")
    os.environ["LASR_TRAINER_GRAPH"] = "1"
    try:
        return _fit(dev, corpus, tmp_path_factory.mktemp("fused"), "bf16", ema_decay=0.9)
    finally:
        if old is None:
            os.environ.pop("LASR_TRAINER_GRAPH", None)
        else:
            os.environ["LASR_TRAINER_GRAPH"] = old


@pytest.fixture(scope="module")
def plain_fit(dev, corpus, tmp_path_factory):
    return _fit(dev, corpus, tmp_path_factory.mktemp("plain"), "bf16", n_batches=2)


def test_trainer_ema_on_the_fused_route(dev, corpus, fused_fit):
    tr, model, _ = fused_fit
    assert tr.fused is not None and tr.fused.ts.ema is tr._opt.ema and tr.fused.ts.ema_state is tr._opt.ema_state
    assert tr.fused.graph_steps > 0                     # the average was also advanced by replayed graphs
    _check_ema_fit(dev, corpus, tr, model, 8, "bf16")


def test_trainer_ema_on_the_autograd_route(dev, corpus, tmp_path):
    from lightning_asr_amd.train import LightingModule

    class Custom(LightingModule):                       # a module that overrides training_step keeps the autograd loop
        def training_step(self, batch, batch_idx):
            return super().training_step(batch, batch_idx)
    tr, model, _ = _fit(dev, corpus, tmp_path / "run", "f32", cls=Custom, n_batches=2, ema_decay=0.9)
    assert tr.fused is None
    _check_ema_fit(dev, corpus, tr, model, 2, "f32")


def test_trainer_ema_eval_off_validates_the_live_model(dev, corpus, tmp_path):
    tr, model, _ = _fit(dev, corpus, tmp_path / "run", "bf16", n_batches=3, ema_decay=0.9, ema_eval=False)
    ckpt = torch.load(os.path.join(tr.root, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=False)
    assert "ema_state_dict" in ckpt and tr._opt.ema_num_updates == 3
    recorded, v_live = tr.history[-1]["val_loss"], _validate_loaded(dev, corpus, ckpt["state_dict"], "bf16")
    assert abs(recorded - v_live) <= 8 * 2.0 ** -23 * abs(recorded), (recorded, v_live)         # (as in _check_ema_fit)
    assert abs(recorded - _validate_loaded(dev, corpus, ckpt["ema_state_dict"], "bf16")) > 1000 * 2.0 ** -23 * abs(recorded)


def test_trainer_without_ema_writes_neither_key(plain_fit):
    tr, model, _ = plain_fit
    ckpt = torch.load(os.path.join(tr.root, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=False)
    assert "ema_state_dict" not in ckpt and "ema" not in ckpt
    assert tr._opt.ema is None and tr._opt.ema_state is None
    assert set(ckpt["optimizer_states"][0]["lasr"]) == {"exp_avg", "exp_avg_sq"}
    assert tr.fused.ts.ema is None


# ---- 8. predict ----------------------------------------------------------------------------------------------------------------
def test_translator_picks_the_averaged_weights(dev, fused_fit, plain_fit):
    from lightning_asr_amd.predict import AsrTranslator
    tr, model, _ = fused_fit
    path = os.path.join(tr.root, "checkpoints", "last.ckpt")
    live, ema = model.encoder.native.params, tr._opt.ema
    assert not _same_bits(live, ema)
    for use_ema, want in ((None, ema), (True, ema), (False, live)):
        t = AsrTranslator(path, map_location=str(dev), labels=LABELS, use_ema=use_ema)
        assert _same_bits(t.model.encoder.native.params, want), use_ema
        assert _same_bits(t.model.encoder.native.buffers, model.encoder.native.buffers)
    assert _same_bits(AsrTranslator(path, map_location=str(dev), labels=LABELS).model.encoder.native.params, ema)
    tr0, model0, _ = plain_fit
    path0 = os.path.join(tr0.root, "checkpoints", "last.ckpt")
    with pytest.raises(ValueError, match="use_ema"):
        AsrTranslator(path0, map_location=str(dev), labels=LABELS, use_ema=True)
    for use_ema in (None, False):
        t = AsrTranslator(path0, map_location=str(dev), labels=LABELS, use_ema=use_ema)
        assert _same_bits(t.model.encoder.native.params, model0.encoder.native.params)
