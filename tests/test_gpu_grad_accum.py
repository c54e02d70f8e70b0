"""GPU tier of gradient accumulation (accumulate_grad_batches = K): the accumulate kernel bit for bit against torch's add, a window
of TrainStep(accumulate=K) bit for bit against the same window driven by hand with the K = 1 primitives, the f64 / CPU oracles,
the two graph roles, Trainer.fit on both routes, and the no-sync rule of the staged data-parallel step."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
LABELS = [c.strip() for c in open(os.path.join(ROOT, "data", "labels.txt")).readlines()]
B, L, S = 2, 16000, 5              # T_in = 101


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 255, 256, 257, 16389, 70001)


def _range_sets(n):
    sets = [None, [(0, n)]]
    if n >= 2:
        sets.append([(1, 2)])
    if n >= 3:
        sets.append([(3, 3)])
    if n >= 4100:
        sets += [[(5, 1029), (1029, 4100)], [(7, 11), (4097, n)]]
    return sets


@pytest.mark.parametrize("off_acc, off_g", [(0, 0), (1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_kernel_is_torch_add_bit_for_bit(dev, n, off_acc, off_g):
    """bases sliced as flat[1:] break the 16-byte alignment of both buffers (vector body behind a head) or of one only (the 4-byte
    path); everything outside the ranges - and outside the slice - keeps its bits"""
    from lightning_asr_amd import ops
    gen = torch.Generator().manual_seed(1000 * n + 10 * off_acc + off_g)
    for ranges in _range_sets(n):
        flat_a = torch.randn(n + 9, generator=gen).to(dev)
        flat_g = (torch.randn(n + 9, generator=gen) * 3).to(dev)
        acc, g = flat_a[off_acc:off_acc + n], flat_g[off_g:off_g + n]
        assert (acc.data_ptr() % 16 == 0) == (off_acc == 0) and (g.data_ptr() % 16 == 0) == (off_g == 0)
        want_flat, g_before = flat_a.clone(), flat_g.clone()
        want = want_flat[off_acc:off_acc + n]
        for lo, hi in (ranges if ranges is not None else [(0, n)]):
            want[lo:hi] = acc[lo:hi] + g[lo:hi]
        ops.grad_accumulate(acc, g, ranges)
        torch.cuda.synchronize()
        assert torch.equal(_bits(flat_a), _bits(want_flat)), (n, ranges)
        assert torch.equal(_bits(flat_g), _bits(g_before))


def test_accumulate_kernel_special_values_and_arguments(dev):
    from lightning_asr_amd import _lib, ops
    # signed zeros, denormals, infinities: still torch's add, bit for bit
    a = torch.tensor([0.0, -0.0, -0.0, 1e-45, 3e38, float("inf"), 1.0, -1.0, 16777216.0], device=dev)
    g = torch.tensor([-0.0, -0.0, 0.0, 1e-45, 3e38, 1.0, 5.9604645e-08, 1.0, 1.0], device=dev)
    want = a + g
    ops.grad_accumulate(a, g)
    assert torch.equal(_bits(a), _bits(want))
    # n == 0: nothing to do, no error
    e = torch.empty(0, device=dev)
    ops.grad_accumulate(e, e.clone())
    ops.grad_accumulate(a, g, [])
    x, y = torch.ones(64, device=dev), torch.ones(64, device=dev)
    with pytest.raises(ValueError):
        ops.grad_accumulate(x, y, [(5, 4)])                          # lo > hi
    with pytest.raises(ValueError):
        ops.grad_accumulate(x, y, [(i, i + 1) for i in range(9)])    # nine ranges
    with pytest.raises(ValueError):
        ops.grad_accumulate(x, y, [(0, 65)])                         # past the buffer
    with pytest.raises(ValueError):
        ops.grad_accumulate(x, y[:63])
    with pytest.raises(_lib.LasrError):
        ops.grad_accumulate(x.cpu(), y.cpu())
    with pytest.raises(TypeError):
        ops.grad_accumulate(x.half(), y.half())
    assert float(x.sum()) == 64.0                                    # no refused call wrote anything
    ops.grad_accumulate(x, y, [(i, i + 1) for i in range(8)])        # eight ranges are fine
    assert x.tolist() == [2.0] * 8 + [1.0] * 56


# ---- 2.-4. a window against the same window driven by hand -----------------------------------------------------------------
def _model(dev, variant, dtype, seed=5):
    from lightning_asr_amd.engine import NativeModel
    m = NativeModel(variant, 28, mask=True, act="relu", dtype=dtype, device=dev)
    m.init_parameters(seed=seed)
    return m


def _schedule():
    from lightning_asr_amd.schedule import CosineAnnealingWarmupRestarts
    return CosineAnnealingWarmupRestarts(None, first_cycle_steps=100, cycle_mult=2, max_lr=1e-2, min_lr=1e-4, warmup_steps=3, gamma=0.5)


def _batches(dev, n, base=300):
    out = []
    for s in range(n):
        wave, tg, tl = R.synth_batch(B, L, S, 27, seed=base + s)
        out.append((wave.to(dev), tg.to(dev), tl.to(dev)))
    return out


def _state(m, exp_avg, exp_avg_sq, lr_dev):
    return {"params": m.params.clone(), "buffers": m.buffers.clone(), "exp_avg": exp_avg.clone(), "exp_avg_sq": exp_avg_sq.clone(),
            "lr_dev": lr_dev.clone()}


def _by_hand(dev, variant, dtype, windows, K):
    """the K = 1 primitives: loss_backward per micro-batch, the gradients cloned and summed in order with torch, the sum copied
    into m.grads, ops.novograd_step(grad_scale = 1 / K), the schedule stepped once per window"""
    from lightning_asr_amd import ops
    m, sc = _model(dev, variant, dtype), _schedule()
    exp_avg = torch.zeros_like(m.params)
    exp_avg_sq = torch.zeros(len(m.param_infos()), dtype=torch.float32, device=dev)
    lr_dev = torch.tensor([sc.lr], dtype=torch.float32, device=dev)
    offsets = m.param_offsets()
    losses = []
    for win in windows:
        total = None
        for wave, tg, tl in win:
            _, feats, _, pct = ops.mel(wave, None, None, None, True, dtype, want_bft=False, want_btf=True)
            loss = m.loss_backward(feats, pct, tg, tl)[0]
            losses.append(float(loss.item()))
            g = m.grads.clone()
            total = g if total is None else total + g
        m.grads.copy_(total)
        ops.novograd_step(m.params, m.grads, exp_avg, exp_avg_sq, offsets, lr_dev, 0.8, 0.5, 1e-8, 1e-3, grad_scale=1.0 / K)
        lr_dev.fill_(sc.step())
    torch.cuda.synchronize()
    return _state(m, exp_avg, exp_avg_sq, lr_dev), losses


def _by_trainstep(dev, variant, dtype, windows, K):
    from lightning_asr_amd.step import TrainStep
    m = _model(dev, variant, dtype)
    ts = TrainStep(m, 1e-2, 1e-3, schedule=_schedule(), accumulate=K)
    losses = []
    for win in windows:
        for i, (wave, tg, tl) in enumerate(win):
            short = len(win) < K and i == len(win) - 1           # the incomplete window at the end of an epoch is flushed
            losses.append(float(ts.step(wave, tg, tl, last=True if short else None)[0].item()))
    torch.cuda.synchronize()
    return _state(m, ts.exp_avg, ts.exp_avg_sq, ts.lr_dev), losses, ts, m


def _same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), (k, float((a[k].double() - b[k].double()).abs().max()))


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("variant, dtype", [("plain", torch.float32), ("plain", torch.bfloat16), ("context_se", torch.bfloat16)])
def test_window_equals_the_hand_driven_sum_bit_for_bit(dev, variant, dtype, K):
    bs = _batches(dev, 2 * K)
    windows = [bs[:K], bs[K:]]
    want, l0 = _by_hand(dev, variant, dtype, windows, K)
    got, l1, ts, m = _by_trainstep(dev, variant, dtype, windows, K)
    assert l0 == l1
    _same(want, got)
    assert ts.global_step == 2 and ts.micro == 0 and ts.schedule.last_epoch == 2
    assert int(torch.count_nonzero(m.grads)) == 0                      # zero between windows
    assert int(m.state_dict()["encoder.first_cnn.bn.num_batches_tracked"]) == 2 * K      # BatchNorm counts micro-batches


def test_incomplete_window_steps_with_one_over_k(dev):
    """five micro-batches at K = 2, last=True on the fifth: three optimiser steps, the third from ONE micro-batch scaled by 1/2"""
    bs = _batches(dev, 5)
    windows = [bs[0:2], bs[2:4], bs[4:5]]
    want, l0 = _by_hand(dev, "plain", torch.bfloat16, windows, 2)
    got, l1, ts, m = _by_trainstep(dev, "plain", torch.bfloat16, windows, 2)
    assert l0 == l1
    _same(want, got)
    assert ts.global_step == 3 and ts.micro == 0
    assert int(torch.count_nonzero(m.grads)) == 0


def test_same_batch_twice_at_k2_is_one_k1_step(dev):
    """a scale check that does not rest on the implementation's own arithmetic: (g + g) * 0.5 == g exactly in f32, so K = 2 on the
    same batch twice (no dither, no dropout) moves the parameters and the momentum exactly like one K = 1 step on it.  (The BN
    running statistics were updated twice: the buffers differ and are not compared.)"""
    from lightning_asr_amd.step import TrainStep
    (wave, tg, tl), = _batches(dev, 1, base=77)
    for dtype in (torch.float32, torch.bfloat16):
        m1, m2 = _model(dev, "plain", dtype), _model(dev, "plain", dtype)
        ts1 = TrainStep(m1, 1e-2, 1e-3)
        ts2 = TrainStep(m2, 1e-2, 1e-3, accumulate=2)
        ts1.step(wave, tg, tl)
        ts2.step(wave, tg, tl)
        assert ts2.global_step == 0 and ts2.micro == 1 and torch.equal(m2.params, _model(dev, "plain", dtype).params)
        ts2.step(wave, tg, tl)
        torch.cuda.synchronize()
        assert ts1.global_step == ts2.global_step == 1
        assert torch.equal(m1.params, m2.params) and torch.equal(ts1.exp_avg, ts2.exp_avg) and torch.equal(ts1.exp_avg_sq, ts2.exp_avg_sq)
        assert m1._grads_micro is None                     # K = 1 never allocates the second buffer


def test_accumulate_argument_checks(dev):
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    m = _model(dev, "plain", torch.float32)
    for k in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError):
            TrainStep(m, accumulate=k)
    with pytest.raises(ValueError):
        GraphedTrainStep(TrainStep(m, accumulate=2), B, L, S, role="first")
    with pytest.raises(ValueError):
        m.loss_backward(None, None, None, None, grads=torch.zeros(3, device=dev))


# ---- 5. oracles, f32 -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_micro_batches():
    """two different micro-batches of three one-second clips of 16000 / 12000 / 8000 samples (the shapes of
    test_training_step_matches_oracle_f32), as the reference's collated 4-tuples"""
    out = []
    for seed in (11, 12):
        wave, tg, _ = R.synth_batch(3, 16000, 7, 27, seed=seed)
        lens = [16000, 12000, 8000]
        feats = [R.parse_wave(wave[i, :lens[i]].unsqueeze(0)) for i in range(3)]
        out.append(R.collate(feats, [tg[i].tolist() for i in range(3)]))
    return out


def _oracle_step_inputs(dev, mb):
    from lightning_asr_amd import ops
    inputs, targets, pct, tsz = mb
    feats = ops.bct_to_btc(inputs.to(dev).squeeze(1).contiguous(), torch.float32)
    return feats, pct.to(dev, torch.float32).contiguous(), targets.to(dev), tsz.to(dev, torch.int32)


def _oracle_model(dev):
    from lightning_asr_amd.engine import NativeModel
    m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.float32, device=dev)
    m.load_state_dict(R.formula_state("plain", 28))
    return m


def test_accumulated_gradient_matches_the_f64_oracle(dev, oracle_micro_batches):
    """m.grads after two micro-steps of TrainStep(accumulate=3) against g1 + g2 of the f64 oracle"""
    from conftest import e2e_gate, record_measured
    from lightning_asr_amd.step import TrainStep
    from oracle import ref_bf16 as E
    m = _oracle_model(dev)
    ts = TrainStep(m, 1e-2, 1e-3, accumulate=3)
    for mb in oracle_micro_batches:
        ts.step_features(*_oracle_step_inputs(dev, mb))
    torch.cuda.synchronize()
    assert ts.micro == 2 and ts.global_step == 0
    o64 = E.Bf16OracleModel("plain", 28, mask=True, state=R.formula_state("plain", 28), dtype=torch.float64, emulate=False)
    sums = None
    for inputs, targets, pct, tsz in oracle_micro_batches:
        g = E.loss_and_grads(o64, inputs.double(), targets, pct, tsz)[3]
        sums = g if sums is None else [a + b for a, b in zip(sums, g)]
    got = [m.view(t, m.grads).cpu().double() for t in m.param_infos()]
    assert len(got) == len(sums)
    worst = max(((a - b).norm() / (b.norm() + 1e-30)).item() for a, b in zip(got, sums))
    print("grad_accum_2x_f32_grad_rel_l2_vs_f64_oracle = %.3e" % worst)
    record_measured("grad_accum_2x_f32_grad_rel_l2_vs_f64_oracle", worst)
    assert worst < e2e_gate("grad_accum_2x_f32_grad_rel_l2_vs_f64_oracle"), worst


def test_full_window_matches_the_cpu_oracle_window(dev, oracle_micro_batches):
    """a full K = 2 window: the parameters against tests/helpers/accum_oracle.train_window (bound of the single-step test)"""
    import accum_oracle
    from lightning_asr_amd.step import TrainStep
    om = R.OracleModel("plain", 28, mask=True, state=R.formula_state("plain", 28))
    ref_losses, _ = accum_oracle.train_window(om, R.NovogradState(len(om.parameters())), oracle_micro_batches, 2, 1e-2, 1e-3)
    m = _oracle_model(dev)
    ts = TrainStep(m, 1e-2, 1e-3, accumulate=2)
    losses = [float(ts.step_features(*_oracle_step_inputs(dev, mb))[0].item()) for mb in oracle_micro_batches]
    torch.cuda.synchronize()
    assert ts.global_step == 1
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) / abs(b) < 1e-4
    worst = max(((m.view(t).cpu().double() - q.detach().double()).norm() / (q.detach().double().norm() + 1e-30)).item()
                for t, q in zip(m.param_infos(), om.parameters()))
    print("grad_accum window parameters rel l2 vs cpu oracle = %.3e" % worst)
    assert worst < 1e-3, worst


# ---- 6. graph roles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefetch", [False, True])
def test_graph_roles_equal_the_eager_window(dev, prefetch):
    """one captured graph per role (accumulate, boundary), K = 2, bf16, three windows: bit-identical to the eager
    TrainStep(accumulate=2); capture leaves the running sum, the window counter, the step count and the schedule as it found them"""
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    bs = _batches(dev, 6, base=500)

    def make():
        m = _model(dev, "plain", torch.bfloat16, seed=9)
        ts = TrainStep(m, 1e-2, 1e-3, schedule=_schedule(), accumulate=2)
        ts.use_device_schedule()
        return m, ts
    m0, ts0 = make()
    l0 = [float(ts0.step(w, tg, tl)[0].item()) for w, tg, tl in bs]
    m1, ts1 = make()
    ts1.step(*bs[0])                       # capture in the MIDDLE of a window: a running sum and a counter to preserve
    before = {"params": m1.params.clone(), "buffers": m1.buffers.clone(), "grads": m1.grads.clone(), "exp_avg": ts1.exp_avg.clone(),
              "lr_dev": ts1.lr_dev.clone()}
    assert ts1.micro == 1 and int(torch.count_nonzero(m1.grads)) > 0
    graphs = {}
    for role in ("accumulate", "boundary"):
        graphs[role] = GraphedTrainStep(ts1, B, L, S, prefetch=prefetch, want_logp=True, role=role)
        graphs[role].capture(bs[1][0])
    now = {"params": m1.params, "buffers": m1.buffers, "grads": m1.grads, "exp_avg": ts1.exp_avg, "lr_dev": ts1.lr_dev}
    _same(before, now)
    assert ts1.micro == 1 and ts1.global_step == 0 and ts1.schedule.last_epoch == 0
    l1 = [l0[0]]
    feats, pct = ts1.features(bs[1][0])
    for i in range(1, 6):
        w, tg, tl = bs[i]
        g = graphs["boundary" if i % 2 == 1 else "accumulate"]
        if prefetch:
            g.prime(feats, pct)
            out = g.step(bs[(i + 1) % 6][0], tg, tl)
            feats, pct = g.F_cur, g.pct_cur
        else:
            out = g.step(w, tg, tl)
        l1.append(float(out[0].item()))
    torch.cuda.synchronize()
    assert l0 == l1
    assert torch.equal(m0.params, m1.params) and torch.equal(m0.buffers, m1.buffers)
    assert torch.equal(ts0.exp_avg, ts1.exp_avg) and torch.equal(ts0.exp_avg_sq, ts1.exp_avg_sq) and torch.equal(ts0.lr_dev, ts1.lr_dev)
    assert ts1.global_step == 3 and ts1.micro == 0 and ts1.schedule.last_epoch == 3
    assert int(torch.count_nonzero(m1.grads)) == 0
    assert int(m1.state_dict()["encoder.first_cnn.bn.num_batches_tracked"]) == 6


# ---- 7. Trainer.fit ------------------------------------------------------------------------------------------------------
def _corpus(tmp_path, n_train):
    data = tmp_path / "synth"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_data.py"), "--out", str(data), "--n-train", str(n_train),
                    "--n-dev", "4", "--seconds", "2.0"], check=True)
    return data


def _datamodule(data, dev, act):
    from lightning_asr_amd.data_module import LibriDataModule
    return LibriDataModule([str(data / "train.json")], str(data / "dev.json"), str(data / "dev.json"), LABELS, train_bs=4, dev_bs=4,
                           num_worker=2, device=str(dev), act_dtype=act, train_crop=False)


@pytest.mark.parametrize("n_batches, steps", [(8, 4), (5, 3)])
def test_trainer_fit_accumulates_on_the_fused_route(dev, tmp_path, monkeypatch, n_batches, steps):
    """Trainer(accumulate_grad_batches=2): global_step counts optimiser steps, the schedule's length too, graphs replay both roles,
    and the run lands bit for bit where a hand-driven TrainStep(accumulate=2) lands on the batches the loop saw"""
    from lightning_asr_amd import ops
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.lightning_compat import Trainer, seed_everything
    from lightning_asr_amd.schedule import CosineAnnealingWarmupRestarts
    from lightning_asr_amd.step import TrainStep
    from lightning_asr_amd.train import LightingModule
    monkeypatch.setenv("LASR_TRAINER_GRAPH", "1")
    data = _corpus(tmp_path, 4 * n_batches)
    seed_everything(0)
    dm = _datamodule(data, dev, torch.bfloat16)
    model = LightingModule(learning_rate=1e-2, weight_decay=1e-3, labels=LABELS, total_epoch=1, drop_rate=0.0, mask=True, use_cer=True,
                           dtype="bf16", device=str(dev), warmup_steps=2)
    init = {"params": model.encoder.native.params.clone(), "buffers": model.encoder.native.buffers.clone()}
    seen, steps_at_batch_end = [], []

    def hook(db):
        seen.append({"pcm": db.pcm.clone(), "lens": db.lens.clone(), "targets": db.targets.clone(), "sizes": db.sizes.clone(),
                     "aug": None if db.aug is None else db.aug.clone(), "L": db.L})

    class PerBatch:
        def on_train_batch_end(self, tr):
            steps_at_batch_end.append(tr.global_step)
    tr = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "run"), device=str(dev), check_val_every_n_epoch=1, log_every_n_steps=2,
                 accumulate_grad_batches=2, callbacks=[PerBatch()])
    tr._fused_on_batch = hook
    tr.fit(model, dm)
    assert tr.fused is not None and tr.fused.ts.accumulate == 2
    assert tr.global_step == steps and tr.fused.ts.global_step == steps and len(seen) == n_batches
    assert steps_at_batch_end == [(i + 1) // 2 if i + 1 < n_batches else steps for i in range(n_batches)]     # the hook stays per batch
    assert tr.fused.ts.schedule.first_cycle_steps == steps
    if n_batches == 8:
        assert tr.fused.graph_steps > 0 and {k[1] for k, g in tr.fused.graphs.items() if g.graph is not None} == {False, True}
    m2 = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
    m2.params.copy_(init["params"]); m2.buffers.copy_(init["buffers"])
    sched = CosineAnnealingWarmupRestarts(None, first_cycle_steps=steps, cycle_mult=2, max_lr=1e-2, min_lr=1e-4, warmup_steps=2, gamma=0.5)
    ts = TrainStep(m2, 1e-2, 1e-3, schedule=sched, accumulate=2)
    dd = ops.DeviceDither(tr.fused.dither.seed, dev)
    for i, b in enumerate(seen):
        nxt = seen[i + 1] if i + 1 < len(seen) else None
        ts.step(b["pcm"], b["targets"], b["sizes"], sample_lens=b["lens"], dither=dd, aug=b["aug"],
                prefetch_wave=None if nxt is None else nxt["pcm"], prefetch_lens=None if nxt is None else nxt["lens"],
                prefetch_dither=None if nxt is None else dd, prefetch_aug=None if nxt is None else nxt["aug"], want_logp=False,
                logical_len=b["L"], prefetch_logical_len=None if nxt is None else nxt["L"], last=nxt is None)
    torch.cuda.synchronize()
    assert ts.global_step == steps
    assert torch.equal(model.encoder.native.params, m2.params), float((model.encoder.native.params - m2.params).abs().max())
    assert torch.equal(model.encoder.native.buffers, m2.buffers)


def _keep(t):
    """a copy of a batch entry that outlives the loader's buffers (with the channels-last twin the mel kernel attached)"""
    if not torch.is_tensor(t):
        return t
    c = t.clone()
    if getattr(t, "_lasr_btf", None) is not None:
        c._lasr_btf = t._lasr_btf.clone()
    return c


def test_trainer_fit_accumulates_on_the_autograd_route(dev, tmp_path, monkeypatch):
    """a module that overrides training_step keeps the autograd loop: K = 2 over five batches is three Novograd.step calls and the
    parameters of a hand loop of zero_grad / (loss / 2).backward() x 2 / step over the batches the module saw"""
    from lightning_asr_amd.lightning_compat import Trainer, seed_everything
    from lightning_asr_amd.scheduler.novograd import Novograd
    from lightning_asr_amd.train import LightingModule
    data = _corpus(tmp_path, 20)
    seed_everything(0)
    dm = _datamodule(data, dev, torch.float32)
    seen = []

    class Custom(LightingModule):
        def training_step(self, batch, batch_idx):
            seen.append(tuple(_keep(t) for t in batch))
            return super().training_step(batch, batch_idx)
    kw = dict(learning_rate=1e-2, weight_decay=1e-3, labels=LABELS, total_epoch=1, drop_rate=0.0, mask=True, use_cer=True, dtype="f32",
              device=str(dev), warmup_steps=2)
    model = Custom(**kw)
    init = {"params": model.encoder.native.params.clone(), "buffers": model.encoder.native.buffers.clone()}
    calls = []
    real_step = Novograd.step
    monkeypatch.setattr(Novograd, "step", lambda self, closure=None: (calls.append(1), real_step(self, closure))[1])
    tr = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "run"), device=str(dev), accumulate_grad_batches=2,
                 check_val_every_n_epoch=2)              # (no validation pass: this test is about the training loop)
    tr.fit(model, dm)
    assert tr.fused is None and len(seen) == 5
    assert len(calls) == 3 and tr.global_step == 3
    model2 = LightingModule(**kw)
    n2 = model2.encoder.native
    n2.params.copy_(init["params"]); n2.buffers.copy_(init["buffers"])
    model2.trainer = tr
    opts, scheds = model2.configure_optimizers()
    opt, sched = opts[0], scheds[0]["scheduler"]
    assert sched.first_cycle_steps == 3
    model2.train()
    for lo in (0, 2, 4):
        opt.zero_grad()
        for i in range(lo, min(lo + 2, 5)):
            (model2.training_step(seen[i], i) / 2).backward()
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    assert len(calls) == 6
    assert torch.equal(model.encoder.native.params, n2.params), float((model.encoder.native.params - n2.params).abs().max())
    assert torch.equal(model.encoder.native.buffers, n2.buffers)


def test_second_backward_without_zero_grad_adds(dev):
    """torch semantics on the autograd route: loss.backward() twice without zero_grad() leaves p.grad = the sum of the two single
    gradients (bit-equal to torch's add of the two clones); after zero_grad() a backward overwrites again"""
    from lightning_asr_amd.scheduler.novograd import Novograd
    from lightning_asr_amd.train import LightingModule
    m = LightingModule(learning_rate=1e-2, weight_decay=1e-3, labels=LABELS, total_epoch=1, drop_rate=0.0, mask=True, use_cer=True,
                       device=str(dev))
    m.train()
    native = m.encoder.native
    opt = Novograd(m.parameters(), lr=1e-2, weight_decay=1e-3, betas=(0.8, 0.5))
    gen = torch.Generator().manual_seed(4)
    batches = []
    for _ in range(2):
        x = torch.randn(2, 1, 64, 101, generator=gen).to(dev)
        tg = torch.randint(0, 27, (2, 4), generator=gen).to(dev)
        batches.append((x, tg, torch.tensor([1.0, 0.8], device=dev), torch.tensor([4, 3], dtype=torch.int32, device=dev)))
    singles = []
    for b in batches:
        opt.zero_grad()
        m._shared(b)[1].backward()
        singles.append(native.grads.clone())
    assert native._grads_micro is None                             # single backwards never touch the second buffer
    assert not torch.equal(singles[0], singles[1])
    opt.zero_grad()
    m._shared(batches[0])[1].backward()
    assert torch.equal(_bits(native.grads), _bits(singles[0]))
    m._shared(batches[1])[1].backward()                            # no zero_grad: adds
    torch.cuda.synchronize()
    assert torch.equal(_bits(native.grads), _bits(singles[0] + singles[1]))
    for p, t in zip(m.parameters(), native.param_infos()):
        assert p.grad is not None and p.grad.data_ptr() == native.grads.data_ptr() + 4 * t.offset
    opt.zero_grad()
    m._shared(batches[1])[1].backward()
    assert torch.equal(_bits(native.grads), _bits(singles[1]))


# ---- 8. no-sync, one rank ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant, n_buckets", [("plain", 2), ("plain", 4), ("context_se", 2), ("context_se", 4)])
def test_staged_window_all_reduces_on_boundaries_only(dev, variant, n_buckets, monkeypatch):
    """the staged step on a 1-rank communicator (the all-reduce is the identity) against the same staging with the collectives
    left out: bit-identical trajectories over two K = 2 windows, and exactly one set of bucket collectives per optimiser step"""
    from lightning_asr_amd.comm import Communicator
    from lightning_asr_amd.step import TrainStep
    monkeypatch.setenv("LASR_DP_BUCKETS", str(n_buckets))
    bs = _batches(dev, 4, base=700)

    class NoComm:                      # same staging, no collectives
        world, rank = 1, 0
        calls = 0

        def all_reduce_ranges(self, flat, ranges):
            NoComm.calls += 1

        def broadcast(self, flat, root=0):
            pass

        def wait(self):
            pass

    def run(comm):
        m = _model(dev, variant, torch.bfloat16)
        ts = TrainStep(m, 1e-2, 1e-3, comm=comm, accumulate=2)
        ts.force_staged = True
        losses = [float(ts.step(w, tg, tl)[0].item()) for w, tg, tl in bs]
        torch.cuda.synchronize()
        assert ts.global_step == 2 and int(torch.count_nonzero(m.grads)) == 0
        return {"params": m.params.clone(), "buffers": m.buffers.clone(), "exp_avg": ts.exp_avg.clone()}, losses
    s0, l0 = run(NoComm())
    assert NoComm.calls == n_buckets * 2
    comm = Communicator.single(dev)
    s1, l1 = run(comm)
    comm.close()
    assert l0 == l1
    _same(s0, s1)


# ---- 9. two ranks ----------------------------------------------------------------------------------------------------------
def _dp_batch(rank, micro):
    return R.synth_batch(B, L, S, 27, seed=900 + 10 * micro + rank)


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lightning_asr_amd.engine import NativeModel
        from lightning_asr_amd.step import TrainStep
        dev = torch.device("cuda", 0)
        m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.float32, device=dev)
        m.init_parameters(seed=rank)                 # ranks start apart: the wrap-time broadcast aligns them
        ts = TrainStep(m, 1e-2, 1e-3, accumulate=2)
        assert ts.world == 2 and ts.overlap and ts.comm is None
        ts.broadcast_parameters()
        for micro in range(4):
            wave, tg, tl = _dp_batch(rank, micro)
            ts.step(wave.to(dev), tg.to(dev), tl.to(dev))
        torch.cuda.synchronize()
        q.put((rank, m.params.cpu().numpy(), ts.global_step))
    except Exception:
        import traceback
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_accumulate_then_average(dev):
    """two ranks (gloo over one GPU, as in test_gpu_dp.py), K = 2, two windows, f32: the replicas stay bit-identical and land
    where one process lands that sums the four gradients of a window (2 ranks x 2 micro-batches, all taken at the window's
    parameters) and steps with grad_scale 1 / (K world).  Bound: the staged and the single-call backward are the same sums in f32
    up to their order, so the parameters agree to f32 round-off - relative L2 1e-6, the bound test_gpu_dp.py carries for K = 1."""
    import torch.multiprocessing as mp
    from lightning_asr_amd import ops
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in res:
        assert r[1] is not None, r[2]
    assert res[0][2] == res[1][2] == 2
    got = [torch.from_numpy(r[1]) for r in res]
    assert torch.equal(got[0], got[1])
    m = _model(dev, "plain", torch.float32, seed=0)
    exp_avg = torch.zeros_like(m.params)
    exp_avg_sq = torch.zeros(len(m.param_infos()), dtype=torch.float32, device=dev)
    lr_dev = torch.tensor([1e-2], dtype=torch.float32, device=dev)
    for window in range(2):
        total = torch.zeros_like(m.grads)
        for rank in range(2):
            for micro in (2 * window, 2 * window + 1):
                wave, tg, tl = _dp_batch(rank, micro)
                _, feats, _, pct = ops.mel(wave.to(dev), None, None, None, True, torch.float32, want_bft=False, want_btf=True)
                m.loss_backward(feats, pct, tg.to(dev), tl.to(dev))
                total += m.grads
        m.grads.copy_(total)
        ops.novograd_step(m.params, m.grads, exp_avg, exp_avg_sq, m.param_offsets(), lr_dev, 0.8, 0.5, 1e-8, 1e-3, grad_scale=0.25)
    ref = m.params.cpu().double()
    rel = ((got[0].double() - ref).norm() / ref.norm()).item()
    print("two ranks, K = 2: parameters rel l2 vs the single-process sum = %.3e" % rel)
    assert torch.isfinite(got[0]).all() and rel < 1e-6, rel
