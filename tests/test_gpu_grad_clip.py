"""GPU tier of gradient clipping and the non-finite guard ("Gradient clipping and the non-finite guard"): a record in mode
"off" changes no bit, value clipping bit for bit against torch.clamp + today's step, norm clipping against today's step (coef == 1),
the host twin (coef) and an f64 oracle, the guard at every place a NaN can hide, the model's training step (plain, graph-replayed,
accumulating, staged) on a batch whose CTC loss is infinite, and Trainer.fit with its checkpoints."""
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

STEPS, DECAY = 12, 0.5
SCALE = 0.5                        # grad_scale: a power of two, so that g^ = SCALE * g is randn * (0.1 + k) exactly
HYPER = (0.8, 0.5, 1e-8, 1e-3)     # beta1, beta2, eps, weight decay
STATE = ("p", "m", "v", "e")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- tensor tables -------------------------------------------------------------------------------------------------------------
def _offsets(table):
    if table == "many":            # 300 tensors of 1 .. 7 elements: more tensors than the one-workgroup moment kernel has threads
        sizes = np.random.default_rng(300).integers(1, 8, 300)
        return [0] + np.cumsum(sizes).tolist()
    return [0, 1, 4, 9, 16, 21, 1045, table]      # tests/test_gpu_ema.py: boundaries off multiples of 4, a norm chunk's end inside a tensor


TABLES = [1046, 16389, 70001, "many"]
_INPUTS = {}


def _inputs(dev, table):
    """the table, the start and the twelve gradients of a table - made once and left alone"""
    if table not in _INPUTS:
        offs = _offsets(table)
        n = offs[-1]
        g = torch.Generator().manual_seed(4242 + n)
        p0 = torch.randn(n, generator=g).to(dev)
        hat = [torch.randn(n, generator=g) * (0.1 + k) for k in range(STEPS)]              # g^, the scaled gradient
        _INPUTS[table] = {"offs": torch.tensor(offs, dtype=torch.int64, device=dev), "offs_host": offs, "n": n, "n_t": len(offs) - 1, "p0": p0,
                          "hat": [h.to(dev) for h in hat], "grads": [(h / SCALE).to(dev) for h in hat],
                          "lr": torch.tensor([1e-2], dtype=torch.float32, device=dev)}
    return _INPUTS[table]


def _start(dev, inp, keep, ema):
    from lightning_asr_amd import ops
    n_t, p0 = inp["n_t"], inp["p0"]
    return {"p": p0.clone(), "m": torch.zeros_like(p0), "v": torch.zeros(n_t, dtype=torch.float32, device=dev),
            "e": p0.clone() if ema else None, "est": ops.ema_state(DECAY, True, 0, device=dev) if ema else None,
            "ws": ops.novograd_workspace(n_t, inp["n"], dev) if keep else None}


def _clone(s, fresh_ws=False, dev=None, inp=None):
    from lightning_asr_amd import ops
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()}
    if fresh_ws and s["ws"] is not None:
        out["ws"] = ops.novograd_workspace(inp["n_t"], inp["n"], dev)
    return out


def _step(inp, s, grad, grad_scale=SCALE, clip=None):
    from lightning_asr_amd import ops
    ops.novograd_step(s["p"], grad, s["m"], s["v"], inp["offs"], inp["lr"], *HYPER, grad_scale=grad_scale, ws=s["ws"], ema=s["e"],
                      ema_state=s["est"], clip_state=clip)


def _equal(a, b):
    return {x: a[x] is None or _same_bits(a[x], b[x]) for x in STATE}


def _norm64(hat):
    return float(np.sqrt(np.sum(hat.cpu().numpy().astype(np.float64) ** 2)))


CASES = [(t, keep, ema) for t in TABLES for keep in (False, True) for ema in (False, True)]


# ---- 1. off is off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table, keep, ema", CASES)
def test_record_in_mode_off_and_no_record_change_no_bit(dev, table, keep, ema):
    """today's novograd_step against the new entry without a record and against a record in mode "off"; the record's total_norm is
    numpy's f64 sqrt(sum g^^2) rounded to f32 once (2^-23 relative; the f64 accumulation error is far below that)"""
    from lightning_asr_amd import _lib, ops
    from lightning_asr_amd.ops import _p, _stream
    inp = _inputs(dev, table)
    a, b, c = (_start(dev, inp, keep, ema) for _ in range(3))
    ws_b = ops.novograd_workspace(inp["n_t"], inp["n"], dev)
    rec = ops.clip_state("off", device=dev)
    for k in range(STEPS):
        gr = inp["grads"][k]
        _step(inp, a, gr)
        if not keep:
            ws_b.random_(0, 255)                   # a workspace the caller does not keep may hold anything
        _lib.call("lasr_novograd_step_clip", _p(b["p"]), _p(gr), _p(b["m"]), _p(b["v"]), _p(inp["offs"]), inp["n_t"], inp["n"], _p(inp["lr"]),
                  *HYPER, SCALE, _p(b["ws"] if keep else ws_b), ws_b.numel(), _stream(), _p(b["e"]) if ema else None,
                  _p(b["est"]) if ema else None, int(keep), None)
        _step(inp, c, gr, clip=rec)
        torch.cuda.synchronize()
        assert all(_equal(a, b).values()), (k, "no record", _equal(a, b))
        assert all(_equal(a, c).values()), (k, "mode off", _equal(a, c))
        st = ops.clip_state_read(rec)
        want = _norm64(inp["hat"][k])
        assert abs(st["total_norm"] - want) <= 2.0 ** -23 * want, (k, st["total_norm"], want)
        assert st["coef"] == 1.0 and st["last_skipped"] is False
    if ema:
        assert torch.equal(a["est"], b["est"]) and torch.equal(a["est"], c["est"])
    st = ops.clip_state_read(rec)
    assert st["steps"] == STEPS and st["skipped"] == 0 and st["algorithm"] == "off"


# ---- 2. value mode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table, keep, ema", CASES)
def test_value_clip_is_torch_clamp_then_todays_step_bit_for_bit(dev, table, keep, ema):
    from lightning_asr_amd import ops
    inp = _inputs(dev, table)
    c = float(inp["hat"][6].abs().median())        # (an f32 value) steps on both sides of it clip some elements, step 0 none
    top = float(max(h.abs().max() for h in inp["hat"])) * 2.0
    a, b, hi, plain = (_start(dev, inp, keep, ema) for _ in range(4))
    rec, rec_hi = ops.clip_state("value", c, device=dev), ops.clip_state("value", top, device=dev)
    n_clipped = []
    for k in range(STEPS):
        gr = inp["grads"][k]
        clamped = torch.clamp(gr * SCALE, -c, c)
        n_clipped.append(int((clamped != gr * SCALE).sum()))
        _step(inp, a, gr, clip=rec)
        _step(inp, b, clamped, grad_scale=1.0)
        _step(inp, hi, gr, clip=rec_hi)
        _step(inp, plain, gr)
        torch.cuda.synchronize()
        assert all(_equal(a, b).values()), (k, _equal(a, b))
        assert all(_equal(hi, plain).values()), (k, "c above every |g^|", _equal(hi, plain))
        st = ops.clip_state_read(rec)
        want = _norm64(clamped)                    # value mode: the norm of the CLAMPED values
        assert abs(st["total_norm"] - want) <= 2.0 ** -23 * want and st["coef"] == 1.0
    assert n_clipped[0] == 0 and all(x > 0 for x in n_clipped[3:]), n_clipped
    if ema:
        assert torch.equal(a["est"], b["est"])


# ---- 3. norm mode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table, keep, ema", CASES)
def test_norm_clip_against_todays_step_the_host_twin_and_the_f64_oracle(dev, table, keep, ema):
    """Every step starts three paths from the fused path's state: the un-clipped step (bit-equal when coef == 1), the parent's path
    (torch forms (g s) coef in f32, then today's step with grad_scale 1) and the f64 oracle.  The fused path may err against the
    oracle at most twice what the parent's path errs, plus one f32 ulp of max |p|: its per-tensor norm is coef^2 sum g^^2 rather
    than the sum over the rounded products, which can move denom by an ulp.
    Measured on an MI355X (max over the twelve steps, n = 70001, kept workspace, with EMA): fused 2.305e-07, parent's path 2.305e-07
    (the 300-tensor table: 1.192e-07 against 1.194e-07)."""
    import grad_clip_oracle
    from lightning_asr_amd import ops
    inp = _inputs(dev, table)
    c = 5.0 * float(np.sqrt(inp["n"]))
    a = _start(dev, inp, keep, ema)
    rec = ops.clip_state("norm", c, device=dev)
    coefs, worst = [], (0.0, 0.0)
    for k in range(STEPS):
        gr = inp["grads"][k]
        plain, parent = _clone(a, True, dev, inp), _clone(a, True, dev, inp)
        f64 = {x: a[x].cpu().numpy().astype(np.float64) for x in ("p", "m", "v")}
        _step(inp, a, gr, clip=rec)
        st = ops.clip_state_read(rec)
        coef = np.float32(st["coef"])
        coefs.append(float(coef))
        assert coef.tobytes() == ops.clip_coef(st["total_norm"], c).tobytes(), (k, st)
        want = _norm64(inp["hat"][k])              # norm mode: the norm BEFORE the clip
        assert abs(st["total_norm"] - want) <= 2.0 ** -23 * want
        _step(inp, plain, gr)
        _step(inp, parent, (gr * SCALE) * float(coef), grad_scale=1.0)
        torch.cuda.synchronize()
        if coef == 1.0:
            assert all(_equal(a, plain).values()), (k, _equal(a, plain))
        else:
            assert not _same_bits(a["p"], plain["p"])
        info = grad_clip_oracle.step(f64, gr.cpu().numpy(), inp["offs_host"], 1e-2, *HYPER, grad_scale=SCALE, algorithm="norm", clip_val=c)
        assert abs(info["coef"] - float(coef)) <= 2.0 ** -22
        err_fused = float(np.abs(a["p"].cpu().numpy().astype(np.float64) - f64["p"]).max())
        err_parent = float(np.abs(parent["p"].cpu().numpy().astype(np.float64) - f64["p"]).max())
        ulp = float(np.spacing(np.float32(np.abs(f64["p"]).max())))
        print("step %d: coef %.6f, max |p - p_f64|: fused %.3e, parent's path %.3e (ulp of max |p| %.3e)" % (k, coef, err_fused, err_parent, ulp))
        assert err_fused <= 2.0 * err_parent + ulp, (k, float(coef), err_fused, err_parent, ulp)
        worst = (max(worst[0], err_fused), max(worst[1], err_parent))
    print("worst over %d steps: fused %.3e, parent's path %.3e" % (STEPS, worst[0], worst[1]))
    assert coefs[0] == 1.0 and coefs[-1] < 1.0 and sum(x == 1.0 for x in coefs) >= 2 and sum(x < 1.0 for x in coefs) >= 2, coefs


# ---- 4. the guard ----------------------------------------------------------------------------------------------------------------
def _bad_positions(inp):
    offs, n = inp["offs_host"], inp["n"]
    one = next(t for t in range(1, inp["n_t"]) if offs[t + 1] - offs[t] == 1) if inp["n_t"] > 7 else 0
    pos = {0, n - 1, offs[one]}                    # element 0 (a 1-element tensor of the hand-made table), the scalar tail, a 1-element tensor
    pos |= {e for e in (16383, 16384) if e < n}    # both sides of a norm chunk's boundary
    return sorted(pos)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("table", TABLES)
def test_guard_skips_a_nonfinite_step_wherever_the_value_hides(dev, table, keep):
    from lightning_asr_amd import ops
    inp = _inputs(dev, table)
    c_norm, c_val = 5.0 * float(np.sqrt(inp["n"])), float(inp["hat"][6].abs().median())
    base = _start(dev, inp, keep, True)
    for k in range(2):                             # two finite steps first: the moments and the average are not at their start
        _step(inp, base, inp["grads"][k])
    torch.cuda.synchronize()
    cases = [(alg, bad) for alg in ("off", "norm") for bad in (float("nan"), float("inf"), -float("inf"))] + [("value", float("nan"))]
    for pos in _bad_positions(inp):
        for alg, bad in cases:
            s = _clone(base, True, dev, inp)
            rec = ops.clip_state(alg, {"off": 0.0, "norm": c_norm, "value": c_val}[alg], True, device=dev)
            gr = inp["grads"][2].clone()
            gr[pos] = bad
            _step(inp, s, gr, clip=rec)
            torch.cuda.synchronize()
            st = ops.clip_state_read(rec)
            assert all(_equal(s, base).values()) and torch.equal(s["est"], base["est"]), (pos, alg, bad, _equal(s, base))
            assert st["steps"] == 1 and st["skipped"] == 1 and st["last_skipped"] is True, (pos, alg, bad, st)
            # the next finite step: the kept workspace was re-zeroed (a NaN left in it would poison this step)
            fresh = _clone(s, True, dev, inp)
            _step(inp, s, inp["grads"][3], clip=rec)
            _step(inp, fresh, inp["grads"][3], clip=ops.clip_state(alg, st["clip_val"], True, device=dev))
            torch.cuda.synchronize()
            assert all(_equal(s, fresh).values()) and bool(torch.isfinite(s["p"]).all()), (pos, alg, bad)
            assert not _same_bits(s["p"], base["p"])
            st = ops.clip_state_read(rec)
            assert st["steps"] == 2 and st["skipped"] == 1 and st["last_skipped"] is False
        # value mode clamps an Inf: a finite step, equal to the torch path
        s, t = _clone(base, True, dev, inp), _clone(base, True, dev, inp)
        rec = ops.clip_state("value", c_val, True, device=dev)
        gr = inp["grads"][2].clone()
        gr[pos] = float("inf")
        _step(inp, s, gr, clip=rec)
        _step(inp, t, torch.clamp(gr * SCALE, -c_val, c_val), grad_scale=1.0)
        torch.cuda.synchronize()
        assert all(_equal(s, t).values()) and ops.clip_state_read(rec)["skipped"] == 0 and bool(torch.isfinite(s["p"]).all()), pos
        # guard off: today's behaviour - the NaN reaches the parameters
        for alg in ("off", "norm"):
            s = _clone(base, True, dev, inp)
            rec = ops.clip_state(alg, {"off": 0.0, "norm": c_norm}[alg], False, device=dev)
            gr = inp["grads"][2].clone()
            gr[pos] = float("nan")
            _step(inp, s, gr, clip=rec)
            torch.cuda.synchronize()
            assert not bool(torch.isfinite(s["p"]).all()) and ops.clip_state_read(rec)["skipped"] == 0, (pos, alg)


def test_novograd_step_refuses_a_foreign_record(dev):
    from lightning_asr_amd import ops
    inp = _inputs(dev, 1046)
    s = _start(dev, inp, False, False)
    for bad in (torch.zeros(8, dtype=torch.uint8, device=dev), torch.zeros(40, dtype=torch.float32, device=dev), ops.clip_state("off", device="cpu")):
        with pytest.raises(ValueError, match="clip_state"):
            _step(inp, s, inp["grads"][0], clip=bad)
    with pytest.raises(ValueError, match="come together"):
        ops.novograd_step(s["p"], inp["grads"][0], s["m"], s["v"], inp["offs"], inp["lr"], ema=s["p"].clone(), clip_state=ops.clip_state("off", device=dev))


# ---- 5. the model ----------------------------------------------------------------------------------------------------------------
B, L, S = 2, 16000, 60             # T_in = 101, hence 51 output frames: a transcript of 60 labels cannot be aligned


def _model(dev, dtype=torch.float32, seed=5):
    from lightning_asr_amd.engine import NativeModel
    m = NativeModel("plain", 28, mask=True, act="relu", dtype=dtype, device=dev)
    m.init_parameters(seed=seed)
    return m


def _schedule():
    from lightning_asr_amd.schedule import CosineAnnealingWarmupRestarts
    return CosineAnnealingWarmupRestarts(None, first_cycle_steps=100, cycle_mult=2, max_lr=1e-2, min_lr=1e-4, warmup_steps=3, gamma=0.5)


@pytest.fixture(scope="module")
def batch(dev):
    wave, tg, _ = R.synth_batch(B, L, S, 27, seed=901)
    bad = torch.tensor([5, 60], dtype=torch.int32)                     # row 1 is infeasible
    good = torch.tensor([5, 20], dtype=torch.int32)
    return wave.to(dev), tg.to(dev), bad.to(dev), good.to(dev)


def _snapshot(ts):
    return {"params": ts.model.params.clone(), "exp_avg": ts.exp_avg.clone(), "exp_avg_sq": ts.exp_avg_sq.clone(), "ema": ts.ema.clone(),
            "ema_state": ts.ema_state.clone()}


def _unchanged(ts, snap):
    now = _snapshot(ts)
    return {k: torch.equal(now[k].contiguous().view(torch.uint8), snap[k].contiguous().view(torch.uint8)) for k in snap}


def test_trainstep_skips_an_infeasible_batch_and_goes_on(dev, batch):
    from lightning_asr_amd import ops
    from lightning_asr_amd.step import TrainStep
    wave, tg, bad, good = batch
    ts = TrainStep(_model(dev), 1e-2, 1e-3, schedule=_schedule(), skip_nonfinite=True, ema_decay=0.5)
    snap, lr0, epoch0 = _snapshot(ts), ts.lr, ts.schedule.last_epoch
    loss = ts.step(wave, tg, bad)[0]
    torch.cuda.synchronize()
    assert float(loss) == float("inf")
    assert all(_unchanged(ts, snap).values()), _unchanged(ts, snap)
    assert ts.global_step == 1 and ts.schedule.last_epoch == epoch0 + 1 and ts.lr != lr0 and ts.skipped_steps == 1 and ts.ema_num_updates == 0
    loss = ts.step(wave, tg, good)[0]
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and bool(torch.isfinite(ts.model.params).all()) and not _same_bits(ts.model.params, snap["params"])
    st = ops.clip_state_read(ts.clip_state)
    assert st["steps"] == 2 and st["skipped"] == 1 and st["last_skipped"] is False and np.isfinite(st["total_norm"])
    assert ts.global_step == 2 and ts.ema_num_updates == 1


def test_without_the_guard_the_same_batch_leaves_nan_in_the_parameters(dev, batch):
    from lightning_asr_amd.step import TrainStep
    wave, tg, bad, _ = batch
    ts = TrainStep(_model(dev), 1e-2, 1e-3, schedule=_schedule(), ema_decay=0.5)
    assert ts.clip_state is None and ts.skipped_steps == 0
    loss = ts.step(wave, tg, bad)[0]
    torch.cuda.synchronize()
    assert float(loss) == float("inf") and not bool(torch.isfinite(ts.model.params).all())


def test_graph_replays_the_decision(dev, batch):
    from lightning_asr_amd import ops
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    wave, tg, bad, good = batch
    ts = TrainStep(_model(dev, torch.bfloat16, seed=9), 1e-2, 1e-3, schedule=_schedule(), skip_nonfinite=True, ema_decay=0.5)
    snap, rec0 = _snapshot(ts), ts.clip_state.clone()
    g = GraphedTrainStep(ts, B, L, S, prefetch=False, want_logp=True)
    g.capture(wave)
    assert torch.equal(ts.clip_state, rec0) and all(_unchanged(ts, snap).values())          # capture left the record as it found it
    loss = g.step(wave, tg, bad)[0]
    torch.cuda.synchronize()
    assert float(loss) == float("inf") and all(_unchanged(ts, snap).values()), _unchanged(ts, snap)
    assert ts.global_step == 1 and ts.skipped_steps == 1
    loss = g.step(wave, tg, good)[0]
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and bool(torch.isfinite(ts.model.params).all()) and not _same_bits(ts.model.params, snap["params"])
    st = ops.clip_state_read(ts.clip_state)
    assert st["steps"] == 2 and st["skipped"] == 1 and ts.global_step == 2 and ts.ema_num_updates == 1


def test_one_bad_micro_batch_skips_its_window(dev, batch):
    from lightning_asr_amd.step import TrainStep
    wave, tg, bad, good = batch
    m = _model(dev)
    ts = TrainStep(m, 1e-2, 1e-3, schedule=_schedule(), accumulate=2, skip_nonfinite=True, ema_decay=0.5)
    snap = _snapshot(ts)
    ts.step(wave, tg, bad)                         # the bad batch first in its window
    ts.step(wave, tg, good)
    torch.cuda.synchronize()
    assert all(_unchanged(ts, snap).values()), _unchanged(ts, snap)
    assert ts.global_step == 1 and ts.micro == 0 and ts.skipped_steps == 1 and int(torch.count_nonzero(m.grads)) == 0
    ts.step(wave, tg, good)
    ts.step(wave, tg, good)
    torch.cuda.synchronize()
    assert ts.global_step == 2 and ts.skipped_steps == 1 and bool(torch.isfinite(m.params).all()) and not _same_bits(m.params, snap["params"])


def test_staged_step_skips_too(dev, batch, monkeypatch):
    from lightning_asr_amd.comm import Communicator
    from lightning_asr_amd.step import TrainStep
    monkeypatch.setenv("LASR_FORCE_OVERLAP", "1")
    wave, tg, bad, good = batch
    comm = Communicator.single(dev)
    try:
        ts = TrainStep(_model(dev), 1e-2, 1e-3, schedule=_schedule(), comm=comm, skip_nonfinite=True, ema_decay=0.5)
        assert ts.force_staged
        snap = _snapshot(ts)
        ts.step(wave, tg, bad)
        torch.cuda.synchronize()
        assert all(_unchanged(ts, snap).values()) and ts.skipped_steps == 1 and ts.global_step == 1
        ts.step(wave, tg, good)
        torch.cuda.synchronize()
        assert ts.skipped_steps == 1 and bool(torch.isfinite(ts.model.params).all()) and not _same_bits(ts.model.params, snap["params"])
    finally:
        comm.close()


# ---- 6. Trainer.fit ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    data = tmp_path_factory.mktemp("clip") / "synth"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synth_data.py"), "--out", str(data), "--n-train", "32",
                    "--n-dev", "4", "--seconds", "2.0"], check=True)
    return data


def _kw():
    return dict(learning_rate=1e-2, weight_decay=1e-3, labels=LABELS, total_epoch=1, drop_rate=0.0, mask=True, use_cer=True, dtype="bf16",
                warmup_steps=2)


def _datamodule(data, dev):
    from lightning_asr_amd.data_module import LibriDataModule
    return LibriDataModule([str(data / "train.json")], str(data / "dev.json"), str(data / "dev.json"), LABELS, train_bs=4, dev_bs=4,
                           num_worker=2, device=str(dev), act_dtype=torch.bfloat16, train_crop=False)


def test_trainer_fit_clips_publishes_and_checkpoints_the_counts(dev, corpus, tmp_path):
    from lightning_asr_amd import ops
    from lightning_asr_amd.lightning_compat import Trainer, seed_everything
    from lightning_asr_amd.train import LightingModule
    seed_everything(0)
    clip = dict(gradient_clip_val=1e-3, gradient_clip_algorithm="norm", track_grad_norm=True)
    tr = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "run"), device=str(dev), limit_train_batches=6, log_every_n_steps=2, **clip)
    tr.fit(LightingModule(device=str(dev), **_kw()), _datamodule(corpus, dev))
    torch.cuda.synchronize()
    opt = tr._opt
    assert tr.fused is not None and tr.fused.ts.clip_state is opt.clip_state and tr.global_step == 6
    cm = tr.callback_metrics
    assert np.isfinite(cm["grad_norm"]) and cm["grad_norm"] > 0 and 0 < cm["grad_clip_coef"] < 1 and cm["skipped_steps"] == 0
    st = ops.clip_state_read(opt.clip_state)
    assert st["algorithm"] == "norm" and st["steps"] == 6 and st["skipped"] == 0 and st["clip_val"] == float(np.float32(1e-3))
    path = os.path.join(tr.root, "checkpoints", "last.ckpt")
    saved = torch.load(path, map_location="cpu", weights_only=False)["optimizer_states"][0]["lasr"]
    assert saved["clip_steps"] == 6 and saved["clip_skipped"] == 0
    # resume: the counts come back, the mode and the value are the new run's
    tr2 = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "resumed"), device=str(dev), resume_from_checkpoint=path,
                  gradient_clip_val=0.5, gradient_clip_algorithm="value", skip_nonfinite_steps=True)
    tr2.fit(LightingModule(device=str(dev), **_kw()), _datamodule(corpus, dev))              # epoch 0 is done: nothing is trained
    st2 = ops.clip_state_read(tr2._opt.clip_state)
    assert st2["steps"] == 6 and st2["skipped"] == 0 and st2["algorithm"] == "value" and st2["clip_val"] == 0.5 and st2["skip_nonfinite"]
    assert tr2._opt.skipped_steps == 0
