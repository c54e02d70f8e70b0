"""GPU tier: the forward BatchNorm finalize made by the kernel that applies the statistics (csrc/bn_slice.h, DESIGN.md §4 "Switches",
LASR_BN_FWD_FINALIZE).  The consumer-side finalize runs the finalize launch's arithmetic in the finalize launch's order, so every
check here is equality of bits, not a tolerance:

* the channel-sliced apply kernel (lasr_bn_act_fwd_partials) against lasr_bn_finalize_partials + lasr_bn_act_fwd on seeded partial
  sums: out, coef, saved, stats and both running statistics;
* the whole training step (tests/switch_probe.py in subprocesses: the switch is read once per process) with the switch on against
  LASR_BN_FWD_FINALIZE=0 at the shapes where the step changes consumer - every reported number identical, and exactly one BN
  profiler bracket less per unit whose finalize moved."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPS, MOM = 1e-3, 0.1
N_PARTS = (1, 7, 8, 9, 16, 63, 129)     # lane tails of the 8 partial lanes; 129: the second 16 x 8 batch of partial_lane_sum


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _branch(br, parts, gamma, beta, rm, rv, C, dev):
    from lightning_asr_amd.ops import _p
    coef = torch.full((2 * C,), float("nan"), device=dev)
    saved = torch.full((2 * C,), float("nan"), device=dev)
    stats = torch.full((2 * C,), float("nan"), device=dev)
    br.partials, br.n_partials = _p(parts), parts.shape[0]
    br.gamma, br.beta, br.running_mean, br.running_var = _p(gamma), _p(beta), _p(rm), _p(rv)
    br.coef, br.saved, br.stats = _p(coef), _p(saved), _p(stats)
    return coef, saved, stats


@pytest.mark.parametrize("rows", [257, 4008])
@pytest.mark.parametrize("C", [64, 256, 1024])
def test_sliced_apply_from_partials_is_the_two_launches_bit_for_bit(dev, C, rows):
    """lasr_gemm_batch_partials' layout ([n_part][sum | sumsq][C] f32) fed from a seeded tensor: lasr_bn_act_fwd_partials against
    lasr_bn_finalize_partials + lasr_bn_act_fwd, with and without the residual branch, relu and swish, and with the main branch's
    rows past each utterance's length zeroed (what the row-masked GEMM leaves; the forward apply itself masks nothing)."""
    from lightning_asr_amd import _lib, ops
    from lightning_asr_amd.ops import _BnBranch, _p, _stream
    call = _lib.call
    B, T = (8, 501) if rows == 4008 else (1, 257)
    g = torch.Generator(device="cpu").manual_seed(1000 * C + rows)
    rnd = lambda *s: torch.randn(*s, generator=g)
    y_full = rnd(B, T, C).to(dev).bfloat16()
    y2 = rnd(B, T, C).to(dev).bfloat16()
    lens = torch.tensor([T - (i % 5) * (T // 14) - 3 for i in range(B)], device=dev)
    y_tail = (y_full * (torch.arange(T, device=dev)[None, :, None] < lens[:, None, None])).contiguous()
    params = [rnd(C).to(dev) for _ in range(4)]             # gamma, beta, gamma2, beta2
    rm0 = [rnd(C).to(dev) * 0.1 for _ in range(2)]
    rv0 = [(torch.rand(C, generator=g) + 0.5).to(dev) for _ in range(2)]
    for n_part in N_PARTS:
        parts = []
        for _ in range(2):                                  # sums ~ N(0, 3), sums of squares in [20, 30): a positive variance
            p = torch.empty(n_part, 2, C)
            p[:, 0] = rnd(n_part, C) * 3.0
            p[:, 1] = 20.0 + 10.0 * torch.rand(n_part, C, generator=g)
            parts.append(p.to(dev).contiguous())
        for has_res in (False, True):
            nb = 2 if has_res else 1
            for y in (y_full, y_tail):
                for act in ("relu", "swish"):
                    got = {}
                    for form in ("two", "one"):
                        rm = [t.clone() for t in rm0]
                        rv = [t.clone() for t in rv0]
                        brs = (_BnBranch * 2)()
                        outs = [_branch(brs[i], parts[i], params[2 * i], params[2 * i + 1], rm[i], rv[i], C, dev) for i in range(nb)]
                        out = torch.full_like(y, float("nan"))
                        tail = ops._bn_tail(y, dict(coef=outs[0][0]), dict(y=y2, coef=outs[1][0]) if has_res else None, act)
                        if form == "two":
                            call("lasr_bn_finalize_partials", brs, nb, C, rows, EPS, MOM, _stream())
                            call("lasr_bn_act_fwd", _lib.C.byref(tail), _p(out), _stream())
                        else:
                            call("lasr_bn_act_fwd_partials", brs, nb, EPS, MOM, _lib.C.byref(tail), _p(out), _stream())
                        torch.cuda.synchronize()
                        got[form] = {"out": out}
                        for i in range(nb):
                            got[form].update({"coef%d" % i: outs[i][0], "saved%d" % i: outs[i][1], "stats%d" % i: outs[i][2],
                                              "running_mean%d" % i: rm[i], "running_var%d" % i: rv[i]})
                    for k, ref in got["two"].items():
                        assert not torch.isnan(ref.float()).any(), (k, n_part, has_res, act)
                        assert torch.equal(_bits(got["one"][k]), _bits(ref)), (k, C, rows, n_part, has_res, act, y is y_tail)


def _run(env_extra, variant="plain", n_class=28, shape=()):
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("LASR_") and k not in ("LASR_LIB_PATH",):
            del env[k]
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_probe.py"), variant, str(n_class)] + [str(a) for a in shape],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (env_extra, out.stderr[-2000:])
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def _same_step_one_bracket_less_per_unit(env, shape, units, variant="plain"):
    on = _run(dict(env), variant=variant, shape=shape)
    off = _run(dict(env, LASR_BN_FWD_FINALIZE="0"), variant=variant, shape=shape)
    pb_on, pb_off = on.pop("prof_brackets"), off.pop("prof_brackets")
    assert on == off, (env, shape, on, off)
    assert pb_off["bn"] - pb_on["bn"] == units, (env, shape, pb_on, pb_off)
    assert {k: v for k, v in pb_on.items() if k != "bn"} == {k: v for k, v in pb_off.items() if k != "bn"}, (pb_on, pb_off)


def _units_without_se(dev, variant):
    """units of the plan whose BatchNorm finalize moves into their consumer: those without an SE layer (every width of the plan is a
    multiple of 64), from the model's own unit and tensor names"""
    from lightning_asr_amd.engine import NativeModel
    m = NativeModel(variant, 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
    names = {t.name for t in m.tensors}
    units = m.unit_names()
    with_se = [u for u in units if any(n.startswith("encoder.%s." % u) and ".se.fc." in n for n in names)]
    return len(units) - len(with_se)


@pytest.mark.parametrize("env,shape", [
    ({}, ()),                                               # the probe's own shape, T' = 201: the sliced apply kernel everywhere
    ({}, (8, 160000, 1, "relu")),                           # T' = 501, ragged: the half-tile depthwise consumer
    ({}, (8, 160000, 1, "swish")),
    ({"LASR_BN_DW_FUSE": "2"}, (32, 160000, 1, "relu")),    # full tiles take the depthwise consumer too
    ({"LASR_BN_DW_FUSE": "0"}, (32, 160000, 1, "relu")),    # never the depthwise consumer
    ({}, (66, 160000, 0, "relu")),                          # 33 066 rows = 130 row tiles: more than 128 partials per column
], ids=["t201", "half-relu", "half-swish", "full-tiles", "unfused", "130-tiles"])
def test_training_step_is_bit_identical_with_the_finalize_in_its_consumer(dev, env, shape):
    units = _units_without_se(dev, "plain")
    assert units == 15                                      # the plain plan: first_cnn, 13 blocks, last_cnn2
    _same_step_one_bracket_less_per_unit(env, shape, units)


def test_context_se_keeps_the_finalize_of_its_se_units(dev):
    units = _units_without_se(dev, "context_se")
    assert 0 < units < 15
    _same_step_one_bracket_less_per_unit({}, (), units, variant="context_se")
