"""Per-unit ("teacher-forced") parity of the "q105" training step, f32 and bf16: the method of tests/test_gpu_units.py on the plan
with residual blocks of five units.  One step runs through the C ABI with a backward stage per unit (so every unit's d(out) / d(in)
can be read from the workspace, and every block is cut inside); then the helper oracle (tests/helpers/q105_oracle.py) recomputes
each of the 52 units from the GPU's own stored inputs and every tensor the unit produced is compared: u, y, y2, out, dx and the
parameter gradients, then the head.

Gates: TOL of tests/test_gpu_units.py:58-62 (relative L2 per tensor) -
    bf16: act 3e-4, grad_act 1.0e-3, grad_param 1.0e-3, logp_abs 2e-5, nll 2e-6
    f32:  act 5e-6, grad_act 6e-4,   grad_param 2e-5,   logp_abs 2e-5, nll 2e-6
imported from there, not restated.

The one new quantity is the gradient into a block's FIRST sub-unit: its depthwise data gradient takes the residual branch's data
gradient dxr = dy2 Wr of the block's CLOSING sub-unit as addend (csrc/model.hip, Unit::res_sink) - stages apart in this test.  Expected:
the oracle's dx of that sub-unit from the GPU's d(out) (bwd.g_prev) PLUS the oracle's residual dx of the same block's closing
sub-unit, stored once (bf16: one rounding of the f32 sum, as the kernel does).  The closing sub-unit's own dx must NOT contain it.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from oracle import ref_bf16 as E          # noqa: E402
from oracle import ref_cpu as R           # noqa: E402
import q105_oracle as Q                   # noqa: E402
from test_gpu_units import TOL, _bct, rel_l2   # noqa: E402

pytestmark = pytest.mark.gpu


def run_units_check_q105(dev, dtype, wave, sample_lens, tg, tl, tag, oracle_dtype, weights, mask=True, drop_p=0.0):
    from lightning_asr_amd import ops
    from lightning_asr_amd.engine import NativeModel
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    mode = "bf16" if dtype == torch.bfloat16 else "f32"
    tol = TOL[mode]
    n_class = 28
    state = Q.random_state(n_class, 0) if weights == "random" else Q.formula_state(n_class)
    m = NativeModel("q105", n_class, mask=mask, act="relu", dtype=dtype, device=dev)
    m.load_state_dict(state)
    if drop_p:
        m.set_dropout(drop_p, seed=12345)
    B = wave.shape[0]
    _, feats, frames, pct = ops.mel(wave.to(dev), None if sample_lens is None else sample_lens.to(dev), None, None, True, dtype,
                                    want_bft=False, want_btf=True)
    names = m.unit_names()
    T = m.out_frames(feats.shape[1])
    N = B * T
    units = {}

    def on_unit(i, name):
        units[name] = {"g_prev": m.tap("bwd.g_prev").clone(), "g_cur": m.tap("bwd.g_cur").clone()}
    loss, nll, logp, am = m.loss_backward_units(feats, pct, tg.to(dev), tl.to(dev), on_unit)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(m.grads).all()
    gpu_grads = {t.name: m.view(t, m.grads).detach().float().cpu() for t in m.param_infos()}
    pct_c = pct.cpu()
    lens = R.mask_lengths(T, pct_c)
    assert m.tap("lens").cpu().tolist() == lens.tolist()
    o = Q.Bf16OracleModel(n_class, mask=mask, state={k: v.clone() for k, v in state.items()}, dtype=oracle_dtype, emulate=(mode == "bf16"))
    chans = {"first_cnn": (64, 256), "last_cnn2": (512, 1024)}
    chans.update({u[0]: (u[2], u[3]) for u in Q.unit_table()})
    worst = {"act": 0.0, "grad_act": 0.0, "grad_param": 0.0}
    over = []

    def note(unit, kind, key, val):
        worst[kind] = max(worst[kind], val)
        if not val < tol[kind]:
            over.append((unit, key, val, tol[kind]))

    def grad_in(name, c):          # d(input of unit `name`) as the GPU left it
        return _bct(units[name]["g_cur"][:N * c].view(B, T, c))
    results = {}
    kept = {}
    for i, name in enumerate(names):
        ci, co = chans[name]
        inner = "." in name
        closing = not inner and name not in ("first_cnn", "last_cnn2")
        x_in = _bct(feats) if i == 0 else _bct(m.tap(names[i - 1]))
        x_block = _bct(m.tap(names[i - 5])) if closing else None          # the input of the block's first sub-unit
        dout = _bct(units[name]["g_prev"][:N * co].view(B, T, co)) if i == len(names) - 1 else grad_in(names[i + 1], co)
        out_gpu = _bct(m.tap(name))
        has_act = not (inner and mask)         # the quirk: with model.mask the inner sub-units have no activation
        drop = None
        if drop_p:
            keep = m.dropout_mask(i, N * co).view(B, T, co).transpose(1, 2).cpu()
            drop = (keep, 1.0 / (1.0 - int(drop_p * 65536 + 0.5) / 65536.0))
            kept[name] = keep.float().mean().item()
            assert abs(kept[name] - (1 - drop_p)) < 5e-3, (name, kept[name])
        r = Q.run_unit(o, name, x_in, lens, dout, act_mask=(out_gpu > 0) if has_act else None, drop=drop, x_block=x_block)
        results[name] = r
        note(name, "act", "out", rel_l2(out_gpu, r["out"]))
        note(name, "act", "y", rel_l2(_bct(m.tap(name + ".y")), r["y"]))
        if "u" in r:
            note(name, "act", "u", rel_l2(_bct(m.tap(name + ".u")), r["u"]))
        if closing:
            note(name, "act", "y2", rel_l2(_bct(m.tap(name + ".y2")), r["y2"]))
        if inner and mask and not drop_p:
            assert bool((out_gpu < 0).any()), name           # no activation between the sub-blocks
        if i > 0 and not name.endswith(".seq.0"):
            note(name, "grad_act", "dx", rel_l2(grad_in(name, ci), r["dx"]))          # (a closing unit's: WITHOUT its residual dx)
        for k, g in r["grads"].items():
            note(name, "grad_param", "d." + k.split("encoder.")[-1], rel_l2(gpu_grads[k], g.float()))
    # the gradient into every block's first sub-unit: its own dx plus the closing sub-unit's residual dx
    for bname, ci, co, k in Q.BLOCKS:
        first = bname + ".seq.0"
        want = results[first]["dx_raw"] + results[bname]["dx_res"]
        if mode == "bf16":
            want = E.rb(want)
        note(first, "grad_act", "dx+dx_res", rel_l2(grad_in(first, ci), want))
        # and it is not small: without the addend the check above fails by orders of magnitude
        assert rel_l2(results[first]["dx"], want) > 10 * tol["grad_act"], (bname, "the residual gradient is negligible here")
    rh = E.run_head(o, _bct(m.tap("last_cnn2")), pct_c, tg, tl, glogits_in=m.tap("grad_logits").cpu())
    lp_err = (logp.cpu().double() - rh["logp"].double()).abs().max().item()
    assert lp_err < tol["logp_abs"], (tag, "logp", lp_err)
    assert ((nll.cpu().double() - rh["nll"].double()).abs() / rh["nll"].double().abs()).max().item() < tol["nll"]
    note("head", "grad_act", "glogits", rel_l2(m.tap("grad_logits").cpu(), rh["glogits"]))
    note("head", "grad_act", "dx", rel_l2(_bct(units["last_cnn2"]["g_prev"][:N * 1024].view(B, T, 1024)), rh["dx"]))
    for k, g in rh["grads"].items():
        note("head", "grad_param", "d." + k, rel_l2(gpu_grads[k], g.float()))
    print("%s: T' = %d, worst act %.2e grad_act %.2e grad_param %.2e (gates %.1e %.1e %.1e)"
          % (tag, T, worst["act"], worst["grad_act"], worst["grad_param"], tol["act"], tol["grad_act"], tol["grad_param"]))
    assert not over, (tag, over[:12])
    return {"T": T, "worst": worst, "kept": kept, "units": names}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_q105_units_b4_t101_formula(dev, dtype):
    wave, tg, tl = R.synth_batch(4, 32000, 12, 27, seed=5)
    lens = torch.tensor([32000, 32000, 28000, 16000], dtype=torch.int32)
    f32 = dtype == torch.float32
    rep = run_units_check_q105(dev, dtype, wave, lens, tg, tl, "q105_b4_t101_" + ("f32" if f32 else "bf16"),
                               torch.float64 if f32 else torch.float32, "formula")
    assert rep["T"] == 101


def test_q105_units_b4_t101_nomask_f32(dev):
    """model.mask = False: the inner sub-units get their activation and stay masked, the closing one is not masked.  End to end this
    model's f32 gradients are 5e-2 from f64 on ANY f32 evaluation (tests/test_gpu_model_q105.py); per unit they are held to 2e-5."""
    wave, tg, tl = R.synth_batch(4, 32000, 12, 27, seed=5)
    lens = torch.tensor([32000, 32000, 28000, 16000], dtype=torch.int32)
    run_units_check_q105(dev, torch.float32, wave, lens, tg, tl, "q105_b4_t101_nomask_f32", torch.float64, "formula", mask=False)


def test_q105_units_b8_t501_ragged_bf16(dev):
    """B = 8, 160 000 samples, ragged as tests/switch_probe.py makes them (100 %, 93 %, ... of the batch's length): T' = 501, where
    the half-tile fused depthwise forms and the channel-sliced BN kernels are taken"""
    B, L = 8, 160000
    wave, tg, tl = R.synth_batch(B, L, 20, 27, seed=77)
    lens = torch.tensor([L - (i % 5) * (L // 14) for i in range(B)], dtype=torch.int32)
    wave = wave * (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1))
    rep = run_units_check_q105(dev, torch.bfloat16, wave, lens, tg, tl, "q105_b8_t501_ragged_bf16", torch.float32, "random")
    assert rep["T"] == 501


def test_q105_units_with_dropout_bf16(dev):
    """drop_rate = 0.1 in every sub-unit and in last_cnn2, against the oracle applying the SAME masks; kept fraction ~ 1 - p per unit"""
    wave, tg, tl = R.synth_batch(6, 48000, 30, 27, seed=21)
    lens = torch.tensor([48000, 48000, 40000, 30000, 48000, 20000], dtype=torch.int32)
    rep = run_units_check_q105(dev, torch.bfloat16, wave, lens, tg, tl, "q105_dropout_bf16", torch.float32, "random", drop_p=0.1)
    assert len(rep["kept"]) == 52
