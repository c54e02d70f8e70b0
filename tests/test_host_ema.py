"""CPU tier of the weight EMA ("Weight EMA"): the host twin of the device weight, the record's host image and its
refusals, the argument checks of Novograd / TrainStep / Trainer that need no device, and which weights of a checkpoint dict load."""
import ctypes
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import ema_oracle  # noqa: E402


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _weight_plain(decay, warmup, t):
    """the definition restated with struct-rounded Python floats: the quotient of two small integers in double, rounded to f32
    once, IS the correctly rounded f32 quotient (the integers are exact in f32, the double quotient is exact to 2^-53)"""
    d = _f32(decay)
    if warmup:
        d = min(d, _f32((1 + t) / (10 + t)))
    return _f32(1.0 - d)              # 1 - d for two f32 in double is exact to 2^-53: one rounding to f32


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.9999])
def test_ema_weight_matches_the_plain_restatement(decay):
    from lightning_asr_amd import ops
    for t in range(41):
        for warmup in (True, False):
            w = ops.ema_weight(decay, warmup, t)
            assert isinstance(w, np.float32)
            assert float(w) == _weight_plain(decay, warmup, t), (decay, warmup, t)
            assert abs((1.0 - float(w)) - ema_oracle.decay_at(decay, warmup, t)) <= 2.0 ** -23


def test_ema_weight_ramp_cap_constant_and_zero_decay():
    from lightning_asr_amd import ops
    # (1 + t) / (10 + t) reaches 0.5 at t = 8: below the cap before, the cap from there on
    assert all(float(ops.ema_weight(0.5, True, t)) > 0.5 for t in range(8))
    assert float(ops.ema_weight(0.5, True, 7)) == _f32(1.0 - _f32(8 / 17))
    assert all(float(ops.ema_weight(0.5, True, t)) == 0.5 for t in range(8, 41))
    assert float(ops.ema_weight(0.5, True, 0)) == _f32(1.0 - _f32(0.1))
    ws = [float(ops.ema_weight(0.9999, True, t)) for t in range(41)]
    assert all(a > b for a, b in zip(ws, ws[1:]))                     # a long decay: still on the ramp, strictly falling
    assert {float(ops.ema_weight(0.9, False, t)) for t in range(41)} == {_f32(1.0 - _f32(0.9))}      # warm-up off: a constant
    assert all(float(ops.ema_weight(0.0, wu, t)) == 1.0 for wu in (True, False) for t in range(41))  # decay 0: the average IS p


def test_ema_state_init_round_trips_and_refuses():
    from lightning_asr_amd import _lib, ops
    lib = _lib.load()
    assert lib.lasr_version() >= 116
    for name in ("lasr_ema_state_bytes", "lasr_ema_state_init", "lasr_novograd_step_ema", "lasr_ema_update"):
        assert name in _lib.SIGNATURES
    nb = int(lib.lasr_ema_state_bytes())
    assert nb == ops.ema_state_bytes() and nb >= struct.calcsize("<qfif")
    for decay, warmup, count in ((0.9, 1, 0), (0.0, 0, 5), (0.9999, 1, 2 ** 40 + 3)):
        buf = ctypes.create_string_buffer(nb)
        assert lib.lasr_ema_state_init(buf, nb, decay, warmup, count) == 0
        got = ops.ema_state_read(buf.raw)
        assert got == {"num_updates": count, "decay": _f32(decay), "warmup": bool(warmup), "w": 0.0}
        assert ops.ema_state_read(ops.ema_state_host(decay, bool(warmup), count)) == got
    E_ARG = -1
    buf = ctypes.create_string_buffer(nb)
    for bad in (float("nan"), 1.0, -0.1, float("inf"), 1.5):
        assert lib.lasr_ema_state_init(buf, nb, bad, 1, 0) == E_ARG, bad
        assert b"decay" in lib.lasr_last_error()
        with pytest.raises(ValueError):
            ops.ema_state_host(bad)
    assert lib.lasr_ema_state_init(buf, nb - 1, 0.9, 1, 0) == E_ARG and b"bytes" in lib.lasr_last_error()       # a short buffer
    assert lib.lasr_ema_state_init(None, nb, 0.9, 1, 0) == E_ARG
    assert lib.lasr_ema_state_init(buf, nb, 0.9, 1, -1) == E_ARG
    with pytest.raises(ValueError):
        ops.ema_state_host(0.9, True, -1)


def test_c_abi_refuses_bad_ema_arguments_before_any_launch():
    from lightning_asr_amd import _lib, ops
    lib = _lib.load()
    E_ARG = -1
    e, p = 0x10000, 0x20000            # never dereferenced: these calls must not reach a launch
    assert lib.lasr_ema_update(e, p, 0, 0.5, None) == 0
    assert lib.lasr_ema_update(None, p, 4, 0.5, None) == E_ARG and b"null" in lib.lasr_last_error()
    assert lib.lasr_ema_update(e, None, 4, 0.5, None) == E_ARG
    assert lib.lasr_ema_update(e, p, -1, 0.5, None) == E_ARG
    assert lib.lasr_ema_update(e, e, 4, 0.5, None) == E_ARG and b"alias" in lib.lasr_last_error()
    assert lib.lasr_ema_update(e, e + 8, 4, 0.5, None) == E_ARG                       # overlapping by half

    def step(ema, state, params=p):
        return lib.lasr_novograd_step_ema(params, 0x30000, 0x40000, 0x50000, 0x60000, 1, 16, 0x70000, 0.8, 0.5, 1e-8, 0.0, 1.0,
                                          0x80000, 1 << 20, None, ema, state, 0)
    assert step(e, None) == E_ARG and b"come together" in lib.lasr_last_error()       # ema without a state
    assert step(None, 0x90000) == E_ARG and b"come together" in lib.lasr_last_error()  # a state without ema
    assert step(p, 0x90000) == E_ARG and b"alias" in lib.lasr_last_error()             # ema aliasing params
    # the Python wrappers refuse CPU tensors, other dtypes and unequal shapes themselves, like grad_accumulate
    with pytest.raises(_lib.LasrError):
        ops.ema_update(torch.zeros(4), torch.zeros(4), 0.5)
    with pytest.raises(TypeError):
        ops.ema_update(torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.float16), 0.5)


@pytest.mark.parametrize("bad", [1.0, -0.5, float("nan"), float("inf"), "0.9", None, True])
def test_novograd_trainstep_and_trainer_refuse_a_bad_ema_decay(bad):
    from lightning_asr_amd.lightning_compat import Trainer
    from lightning_asr_amd.scheduler.novograd import Novograd
    from lightning_asr_amd.step import TrainStep
    with pytest.raises(ValueError):
        Novograd([torch.nn.Parameter(torch.zeros(1))], ema_decay=bad)
    with pytest.raises(ValueError):
        TrainStep(object(), ema_decay=bad)
    with pytest.raises(ValueError):
        Trainer(ema_decay=bad, device="cpu")


def test_trainer_ema_defaults():
    from lightning_asr_amd.lightning_compat import Trainer
    tr = Trainer(device="cpu")
    assert tr.ema_decay == 0.0 and tr.ema_warmup is True and tr.ema_eval is True
    tr = Trainer(device="cpu", ema_decay=0.999, ema_warmup=False, ema_eval=False)
    assert tr.ema_decay == 0.999 and tr.ema_warmup is False and tr.ema_eval is False


def test_select_state_dict_on_hand_made_checkpoints():
    from lightning_asr_amd.lightning_compat import select_state_dict
    live, avg = {"w": torch.zeros(2)}, {"w": torch.ones(2)}
    plain = {"state_dict": live}
    both = {"state_dict": live, "ema_state_dict": avg, "ema": {"decay": 0.9, "warmup": True, "num_updates": 3}}
    assert select_state_dict(plain) is live and select_state_dict(plain, None) is live and select_state_dict(plain, False) is live
    with pytest.raises(ValueError):
        select_state_dict(plain, True)
    with pytest.raises(ValueError):
        select_state_dict({"state_dict": live, "ema_state_dict": None}, True)
    assert select_state_dict(both) is avg and select_state_dict(both, True) is avg and select_state_dict(both, False) is live
    with pytest.raises(ValueError):
        select_state_dict(both, "yes")


def test_oracle_recurrence_and_bound():
    e, trace = ema_oracle.recurrence(np.zeros(2), [np.ones(2), np.ones(2)], [0.5, 0.5])
    assert e.tolist() == [0.75, 0.75] and [t.tolist() for t in trace] == [[0.5, 0.5], [0.75, 0.75]]
    assert ema_oracle.drift_bound(2.0, 0.5) == 5 * 2.0 ** -24 * 2.0 / 0.5
    assert math.isclose(ema_oracle.decay_at(0.9, True, 0), 0.1) and ema_oracle.decay_at(0.9, False, 0) == 0.9
