"""CPU tier of gradient clipping and the non-finite guard ("Gradient clipping and the non-finite guard"): the f64 oracle
against torch's own clipping followed by the reference NovoGrad arithmetic, the record's host image and its refusals, the host twin
of the device coefficient, and the plumbing from the configuration file and the Trainer down to Novograd's arguments."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import grad_clip_oracle  # noqa: E402

OFFSETS = [0, 1, 4, 9, 16, 21, 1045, 1046]


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ["off", "norm", "value"])
def test_oracle_is_torch_clipping_followed_by_the_reference_novograd(algorithm):
    """four steps in f64 on both sides; the clip value is chosen so that early steps pass untouched and late ones are clipped"""
    gen = torch.Generator().manual_seed(11)
    n, n_t = OFFSETS[-1], len(OFFSETS) - 1
    params = [torch.randn(OFFSETS[t + 1] - OFFSETS[t], generator=gen, dtype=torch.float64) for t in range(n_t)]
    state = {"p": torch.cat(params).numpy().copy(), "m": np.zeros(n), "v": np.zeros(n_t)}
    st = R.NovogradState(n_t)
    scale = 0.5
    c = {"off": 0.0, "norm": 2.0 * np.sqrt(n) * scale, "value": 1.5 * scale}[algorithm]
    clipped = []
    for k in range(4):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * (0.1 + k)
        grads = [(g[OFFSETS[t]:OFFSETS[t + 1]] * scale).clone() for t in range(n_t)]
        for p, gr in zip(params, grads):
            p.grad = gr
        if algorithm == "norm":
            total = torch.nn.utils.clip_grad_norm_(params, c)
            clipped.append(bool(float(total) > c))
        elif algorithm == "value":
            clipped.append(bool(max(float(gr.abs().max()) for gr in grads) > c))
            torch.nn.utils.clip_grad_value_(params, c)
        R.novograd_step(params, [p.grad for p in params], st, 1e-2, 0.8, 0.5, 1e-8, 1e-3)
        info = grad_clip_oracle.step(state, g.numpy(), OFFSETS, 1e-2, 0.8, 0.5, 1e-8, 1e-3, grad_scale=scale, algorithm=algorithm,
                                     clip_val=c)
        assert not info["skipped"]
        if algorithm == "norm":
            assert abs(info["total_norm"] - float(total)) <= 1e-12 * float(total)
            assert (info["coef"] < 1.0) == clipped[-1]
        want = torch.cat(params).numpy()
        assert np.abs(state["p"] - want).max() <= 1e-12 * np.abs(want).max(), (k, np.abs(state["p"] - want).max())
        assert np.abs(state["m"] - torch.cat(st.exp_avg).numpy()).max() <= 1e-12 * np.abs(state["m"]).max()
        assert np.abs(state["v"] - torch.stack(st.exp_avg_sq).numpy()).max() <= 1e-12 * np.abs(state["v"]).max()
    if algorithm != "off":
        assert not clipped[0] and clipped[-1]          # both kinds of step occurred


def test_oracle_clamp_keeps_nan_and_guard_leaves_the_state_alone():
    n = OFFSETS[-1]
    state = {"p": np.ones(n), "m": np.full(n, 0.5), "v": np.full(len(OFFSETS) - 1, 2.0)}
    before = {k: v.copy() for k, v in state.items()}
    for bad in (np.nan, np.inf, -np.inf):
        for algorithm in ("off", "norm"):
            g = np.ones(n)
            g[17] = bad
            info = grad_clip_oracle.step(state, g, OFFSETS, 1e-2, algorithm=algorithm, clip_val=1.0, skip_nonfinite=True)
            assert info["skipped"] and all(np.array_equal(state[k], before[k]) for k in state)
    g = np.ones(n)
    g[17] = np.nan
    assert grad_clip_oracle.step(state, g, OFFSETS, 1e-2, algorithm="value", clip_val=0.5, skip_nonfinite=True)["skipped"]
    g[17] = np.inf                                 # clamped to c: a finite step
    info = grad_clip_oracle.step(state, g, OFFSETS, 1e-2, algorithm="value", clip_val=0.5, skip_nonfinite=True)
    assert not info["skipped"] and info["total_norm"] == np.sqrt(n * 0.25) and np.isfinite(state["p"]).all()
    g[17] = np.nan                                 # guard off: the NaN goes through, into the tensor it sits in
    state = {k: v.copy() for k, v in before.items()}
    assert not grad_clip_oracle.step(state, g, OFFSETS, 1e-2, algorithm="norm", clip_val=1.0)["skipped"]
    assert np.isnan(state["p"]).all()              # through coef, into every tensor


# ---- the record ------------------------------------------------------------------------------------------------------------------
def test_clip_state_round_trips_and_refuses():
    from lightning_asr_amd import _lib, ops
    lib = _lib.load()
    assert lib.lasr_version() >= 117
    for name in ("lasr_clip_state_bytes", "lasr_clip_state_init", "lasr_novograd_step_clip"):
        assert name in _lib.SIGNATURES
    nb = int(lib.lasr_clip_state_bytes())
    assert nb == ops.clip_state_bytes() == struct.calcsize(ops._CLIP_STATE_FMT) == 40
    for algorithm, c, guard, steps, skipped in (("off", 0.0, False, 0, 0), ("off", 0.0, True, 5, 1), ("norm", 0.25, True, 2 ** 40 + 3, 7),
                                                ("value", 1e-3, False, 9, 0)):
        got = ops.clip_state_read(ops.clip_state_host(algorithm, c, guard, steps, skipped))
        assert got == {"algorithm": algorithm, "clip_val": _f32(c), "skip_nonfinite": guard, "steps": steps, "skipped": skipped,
                       "total_norm": 0.0, "coef": 1.0, "last_skipped": False}
        buf = ctypes.create_string_buffer(nb)
        assert lib.lasr_clip_state_init(buf, nb, ops.CLIP_MODES[algorithm], c, int(guard), steps, skipped) == 0
        assert ops.clip_state_read(buf.raw) == got
    E_ARG = -1
    buf = ctypes.create_string_buffer(nb)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        for mode in (0, 1, 2):
            assert lib.lasr_clip_state_init(buf, nb, mode, bad, 0, 0, 0) == E_ARG, (mode, bad)
            assert b"clip_val" in lib.lasr_last_error()
        for algorithm in ("off", "norm", "value"):
            with pytest.raises(ValueError):
                ops.clip_state_host(algorithm, bad)
    for mode in (1, 2):                            # a mode without a value
        assert lib.lasr_clip_state_init(buf, nb, mode, 0.0, 0, 0, 0) == E_ARG and b"needs clip_val" in lib.lasr_last_error()
    for algorithm in ("norm", "value"):
        with pytest.raises(ValueError):
            ops.clip_state_host(algorithm, 0.0)
    for mode in (-1, 3):                           # an unknown algorithm
        assert lib.lasr_clip_state_init(buf, nb, mode, 1.0, 0, 0, 0) == E_ARG and b"mode" in lib.lasr_last_error()
    with pytest.raises(ValueError):
        ops.clip_state_host("l2", 1.0)
    assert lib.lasr_clip_state_init(buf, nb, 1, 1.0, 0, -1, 0) == E_ARG           # negative counts
    assert lib.lasr_clip_state_init(buf, nb, 1, 1.0, 0, 0, -1) == E_ARG
    with pytest.raises(ValueError):
        ops.clip_state_host("norm", 1.0, False, -1, 0)
    with pytest.raises(ValueError):
        ops.clip_state_host("norm", 1.0, False, 0, -1)
    assert lib.lasr_clip_state_init(buf, nb - 1, 1, 1.0, 0, 0, 0) == E_ARG and b"bytes" in lib.lasr_last_error()   # a short buffer
    assert lib.lasr_clip_state_init(None, nb, 1, 1.0, 0, 0, 0) == E_ARG


def test_step_clip_refuses_bad_arguments_before_any_launch():
    from lightning_asr_amd import _lib
    lib = _lib.load()
    p = 0x20000                                    # never dereferenced: these calls must not reach a launch

    def step(ema, state, clip):
        return lib.lasr_novograd_step_clip(p, 0x30000, 0x40000, 0x50000, 0x60000, 1, 16, 0x70000, 0.8, 0.5, 1e-8, 0.0, 1.0, 0x80000,
                                           1 << 20, None, ema, state, 0, clip)
    assert step(0x10000, None, 0xA0000) == -1 and b"come together" in lib.lasr_last_error()
    assert step(None, 0x90000, None) == -1 and b"come together" in lib.lasr_last_error()
    assert step(p, 0x90000, 0xA0000) == -1 and b"alias" in lib.lasr_last_error()


def test_clip_coef_is_three_f32_operations():
    from lightning_asr_amd import ops
    rng = np.random.default_rng(3)
    norms = np.concatenate([rng.uniform(0, 4, 200), 10.0 ** rng.uniform(-8, 8, 200), [0.0, 1.0, 1e-6, 1 - 1e-6]]).astype(np.float32)
    for c in (1e-3, 0.25, 1.0, 5.0 * np.sqrt(1046)):
        for N in norms:
            got = ops.clip_coef(N, c)
            assert isinstance(got, np.float32)
            want = np.minimum(np.float32(1.0), np.float32(c) / (N + np.float32(1e-6)))
            assert got.tobytes() == np.float32(want).tobytes(), (c, N)
    assert ops.clip_coef(0.0, 1.0) == 1.0 and ops.clip_coef(np.float32(np.inf), 1.0) == 0.0
    assert np.isnan(ops.clip_coef(np.float32(np.nan), 1.0))                     # guard off: the NaN goes through, as in torch
    assert ops.clip_coef(2.0, 1.0) == np.float32(1.0) / (np.float32(2.0) + np.float32(1e-6))


# ---- the plumbing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(gradient_clip_val=-1.0), dict(gradient_clip_val=float("nan")), dict(gradient_clip_val=float("inf")),
                                dict(gradient_clip_val="1"), dict(gradient_clip_val=True),
                                dict(gradient_clip_val=1.0, gradient_clip_algorithm="l2"),
                                dict(gradient_clip_algorithm=None)])
def test_novograd_trainstep_and_trainer_refuse_bad_clip_settings(kw):
    from lightning_asr_amd.lightning_compat import Trainer
    from lightning_asr_amd.scheduler.novograd import Novograd
    from lightning_asr_amd.step import TrainStep
    name = "gradient_clip_algorithm" if "gradient_clip_algorithm" in kw else "gradient_clip_val"
    with pytest.raises(ValueError, match=name):
        Novograd([torch.nn.Parameter(torch.zeros(1))], **kw)
    with pytest.raises(ValueError, match=name):
        TrainStep(object(), **kw)
    with pytest.raises(ValueError, match=name):
        Trainer(device="cpu", **kw)


def test_trainer_clip_defaults_and_settings():
    from lightning_asr_amd.lightning_compat import Trainer
    tr = Trainer(device="cpu")
    assert (tr.gradient_clip_val, tr.gradient_clip_algorithm, tr.skip_nonfinite_steps, tr.track_grad_norm) == (0.0, "norm", False, False)
    tr = Trainer(device="cpu", gradient_clip_val=1, gradient_clip_algorithm="value", skip_nonfinite_steps=True, track_grad_norm=True)
    assert (tr.gradient_clip_val, tr.gradient_clip_algorithm, tr.skip_nonfinite_steps, tr.track_grad_norm) == (1.0, "value", True, True)
    assert Trainer(device="cpu", gradient_clip_val=None).gradient_clip_val == 0.0            # Lightning's "no clipping"


class _Recorder:
    """stands in for Novograd / the schedule: keeps what it was constructed with"""
    def __init__(self, *args, **kw):
        self.args, self.kw = args, kw


def test_configure_optimizers_hands_the_trainers_settings_to_novograd(monkeypatch):
    """gradient_clip_val used to fall into the Trainer's **ignored: a user who set it got no clipping and no word about it"""
    from lightning_asr_amd import train
    from lightning_asr_amd.lightning_compat import Trainer
    monkeypatch.setattr(train, "Novograd", _Recorder)
    monkeypatch.setattr(train, "CosineAnnealingWarmupRestarts", _Recorder)

    class Module:
        learning_rate, weight_decay, total_epoch, warmup_steps = 1e-2, 1e-3, 1, 2
        print = staticmethod(lambda *a: None)
        parameters = staticmethod(lambda: [])
        train_dataloader = staticmethod(lambda: [0] * 8)
    m = Module()
    m.trainer = Trainer(device="cpu", gradient_clip_val=1.0, gradient_clip_algorithm="value", skip_nonfinite_steps=True,
                        track_grad_norm=True)
    (opt,), _ = train.LightingModule.configure_optimizers(m)
    assert opt.kw["gradient_clip_val"] == 1.0 and opt.kw["gradient_clip_algorithm"] == "value"
    assert opt.kw["skip_nonfinite"] is True and opt.kw["track_grad_norm"] is True
    m.trainer = Trainer(device="cpu")
    (opt,), _ = train.LightingModule.configure_optimizers(m)
    assert opt.kw["gradient_clip_val"] == 0.0 and opt.kw["gradient_clip_algorithm"] == "norm"
    assert opt.kw["skip_nonfinite"] is False and opt.kw["track_grad_norm"] is False


def test_config_file_carries_the_four_keys_to_the_trainer(monkeypatch):
    from lightning_asr_amd import launch, train
    from lightning_asr_amd.config import load_config
    cfg = load_config(os.path.join(ROOT, "conf"), "conf", [])
    t = cfg.get("train")
    assert t.get("gradient_clip_val") == 0 and t.get("gradient_clip_algorithm") == "value"      # what the reference's train.py passes
    assert t.get("skip_nonfinite_steps") is False and t.get("track_grad_norm") is False
    made = {}

    class FakeTrainer(_Recorder):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            made["trainer"] = self

        def fit(self, *a, **k):
            pass

        def test(self, *a, **k):
            pass

    class FakeData(_Recorder):
        def test_dataloader(self):
            return None
    monkeypatch.setattr(train, "Trainer", FakeTrainer)
    monkeypatch.setattr(train, "LibriDataModule", FakeData)
    monkeypatch.setattr(train, "LightingModule", _Recorder)
    monkeypatch.setattr(launch, "maybe_launch", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)
    monkeypatch.delenv("LASR_CONF_DIR", raising=False)
    train.main(["train.gradient_clip_val=0.5", "train.gradient_clip_algorithm=norm", "train.skip_nonfinite_steps=true",
                "train.track_grad_norm=true"])
    kw = made["trainer"].kw
    assert kw["gradient_clip_val"] == 0.5 and kw["gradient_clip_algorithm"] == "norm"
    assert kw["skip_nonfinite_steps"] is True and kw["track_grad_norm"] is True
    train.main([])
    kw = made["trainer"].kw
    assert kw["gradient_clip_val"] == 0.0 and kw["gradient_clip_algorithm"] == "value"
    assert kw["skip_nonfinite_steps"] is False and kw["track_grad_norm"] is False
