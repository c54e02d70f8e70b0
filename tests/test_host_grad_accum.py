"""CPU tier of gradient accumulation (accumulate_grad_batches): the window rule, the Trainer's argument checks, and the CPU oracle of
a window (tests/helpers/accum_oracle.py) against oracle.ref_cpu's single step."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from oracle import ref_cpu as R  # noqa: E402

import accum_oracle  # noqa: E402

T, F = True, False


@pytest.mark.parametrize("n, K, want", [(5, 2, [F, T, F, T, T]), (4, 1, [T] * 4), (1, 4, [T]), (6, 3, [F, F, T, F, F, T])])
def test_window_roles(n, K, want):
    from lightning_asr_amd.fused_fit import window_roles
    assert window_roles(n, K) == want


def test_window_roles_properties():
    from lightning_asr_amd.fused_fit import window_roles
    for n in range(0, 14):
        for K in range(1, 7):
            r = window_roles(n, K)
            assert len(r) == n and sum(r) == -(-n // K)            # ceil(n / K) optimiser steps per epoch
            assert not n or r[-1]                                  # the epoch always ends on a step
    with pytest.raises(ValueError):
        window_roles(4, 0)


@pytest.mark.parametrize("k", [0, -1, 1.5, "2"])
def test_trainer_rejects_a_bad_accumulate_grad_batches(k):
    from lightning_asr_amd.lightning_compat import Trainer
    with pytest.raises(ValueError):
        Trainer(accumulate_grad_batches=k, device="cpu")


def test_trainer_accumulate_grad_batches_dict_and_default():
    from lightning_asr_amd.lightning_compat import Trainer
    with pytest.raises(NotImplementedError):
        Trainer(accumulate_grad_batches={0: 2, 4: 1}, device="cpu")
    assert Trainer(device="cpu").accumulate_grad_batches == 1
    assert Trainer(accumulate_grad_batches=4, device="cpu").accumulate_grad_batches == 4


def _micro_batch(seed, B=2, L=16000, S=4):
    wave, tg, _ = R.synth_batch(B, L, S, 27, seed=seed)
    feats = [R.parse_wave(wave[i].unsqueeze(0)) for i in range(B)]
    return R.collate(feats, [tg[i].tolist() for i in range(B)])          # (inputs, targets, pct, target sizes)


def _oracle():
    return R.OracleModel("plain", 28, mask=True, state=R.formula_state("plain", 28))


@pytest.fixture(scope="module")
def single_steps():
    """R.train_step from the same initial state on two different micro-batches: (batch, loss, grads, parameters after)"""
    out = []
    for seed in (21, 22):
        mb = _micro_batch(seed)
        om = _oracle()
        loss, grads = R.train_step(om, R.NovogradState(len(om.parameters())), *mb, 1e-2, 1e-3)
        out.append((mb, loss, grads, [p.detach().clone() for p in om.parameters()]))
    return out


def test_oracle_window_of_one_is_the_single_step_bit_for_bit(single_steps):
    mb, loss_ref, grads_ref, params_ref = single_steps[0]
    om = _oracle()
    losses, grads = accum_oracle.train_window(om, R.NovogradState(len(om.parameters())), [mb], 1, 1e-2, 1e-3)
    assert losses == [loss_ref]
    assert all(torch.equal(a, b) for a, b in zip(grads, grads_ref))
    assert all(torch.equal(p.detach(), q) for p, q in zip(om.parameters(), params_ref))


def test_oracle_window_of_two_sums_the_halved_gradients(single_steps):
    (mb1, l1, g1, _), (mb2, l2, g2, _) = single_steps
    om = _oracle()
    losses, grads = accum_oracle.train_window(om, R.NovogradState(len(om.parameters())), [mb1, mb2], 2, 1e-2, 1e-3)
    assert losses == [l1, l2]                         # the second forward sees the same parameters: no step in between
    for g, a, b in zip(grads, g1, g2):
        assert torch.allclose(g, (a + b) / 2, rtol=1e-6)
    with pytest.raises(ValueError):
        accum_oracle.train_window(om, R.NovogradState(len(om.parameters())), [mb1, mb2, mb1], 2, 1e-2)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """lasr_grad_accumulate[_ranges]: every refusal, and every call with nothing to add, returns before touching the GPU"""
    import ctypes
    from lightning_asr_amd import _lib
    lib = _lib.load()
    assert lib.lasr_version() >= 114
    assert "lasr_grad_accumulate" in _lib.SIGNATURES and "lasr_grad_accumulate_ranges" in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "lasr.h")).read()
    assert "#define LASR_ACC_MAX_RANGES 8" in text
    from lightning_asr_amd import ops
    assert ops.ACC_MAX_RANGES == 8
    a, g = 0x1000, 0x2000            # never dereferenced: these calls must not reach a launch

    def arr(v):
        return (ctypes.c_int64 * len(v))(*v)

    def ranges(acc, grad, lo, hi, n=None):
        return lib.lasr_grad_accumulate_ranges(acc, grad, arr(lo), arr(hi), len(lo) if n is None else n, None)
    E_ARG = -1
    assert lib.lasr_grad_accumulate(a, g, 0, None) == 0
    assert ranges(a, g, [3], [3]) == 0 and ranges(a, g, [0, 7, 9], [0, 7, 9]) == 0          # only empty ranges
    assert ranges(a, g, [0], [0], n=0) == 0
    assert lib.lasr_grad_accumulate(None, g, 4, None) == E_ARG and lib.lasr_grad_accumulate(a, None, 4, None) == E_ARG
    assert b"null" in lib.lasr_last_error()
    assert lib.lasr_grad_accumulate(a, g, -1, None) == E_ARG
    assert ranges(a, g, [5], [4]) == E_ARG and b"range 0" in lib.lasr_last_error()          # lo > hi
    assert ranges(a, g, [-1], [4]) == E_ARG
    assert ranges(a, g, [0] * 9, [0] * 9) == E_ARG and b"9 ranges" in lib.lasr_last_error()
    assert lib.lasr_grad_accumulate_ranges(a, g, None, arr([1]), 1, None) == E_ARG
    # the Python wrapper refuses CPU tensors itself (there is no CPU path)
    with pytest.raises(_lib.LasrError):
        ops.grad_accumulate(torch.zeros(4), torch.zeros(4))
    with pytest.raises(TypeError):
        ops.grad_accumulate(torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.float16))

