"""CPU oracle of the "q105" variant (MyModel2 with the reference's QuartNet105 encoder, models/QuartNet.py:175-224).  TEST
INFRASTRUCTURE ONLY: the same arithmetic as oracle/ref_cpu.py (f32 / f64) and oracle/ref_bf16.py (bf16 storage emulation) with the
block replaced - ten QuartNetBlock(repeat=5) instead of thirteen QuartNetBlock(repeat=1).

The quirk that is reproduced (models/QuartNet.py:60 against :9): the inner sub-blocks are built as
``SeprationConv(in_ch, in_ch, k, mask, drop_rate=...)``, so the model's ``mask`` lands in the sub-block's ``last`` and the
sub-block's own ``mask`` keeps its default True.  mask=True: no activation between the five sub-blocks, all masked.  mask=False: the
inner sub-blocks have the activation and are STILL masked; only seq.4 (last=True, mask=False) is not.

bf16 storage points of a block (lightning_asr_amd/csrc/model.hip): every sub-unit stores u, y and its output (an inner unit's
output is act(BN(y)) or, with last=True, BN(y) itself); the closing unit stores y2 = Wr x_block and out = act(BN(y) + BN(y2)); in the
backward the residual data gradient dxr = dy2 Wr is its own bf16 tensor, added to the FIRST sub-unit's depthwise data gradient.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_bf16 as E
from oracle import ref_cpu as R

REPEAT = 5
BLOCKS = [("block1", 256, 256, 33), ("block12", 256, 256, 33), ("block2", 256, 256, 39), ("block22", 256, 256, 39),
          ("block3", 256, 512, 51), ("block32", 512, 512, 51), ("block4", 512, 512, 63), ("block42", 512, 512, 63),
          ("block5", 512, 512, 75), ("block52", 512, 512, 75)]

# `gain` of formula_state for the two reference fixtures (tests/golden/model_q105.npz, model_q105_nomask.npz), by model.mask.
# A fixture is a yardstick for an f32 implementation only where the reference's own f32 evaluation reproduces its f64 evaluation:
# the gain is the largest of 1, 0.7, 0.5, 0.35 (steps of 1 / sqrt 2) at which r - the f32 helper oracle's worst per-tensor
# gradient distance from the f64 one, relative L2, at the fixtures' batch - is at most 1e-2, half the cap of the end-to-end gradient
# gate, so that the gate 2 r is set by r and not by its cap.  Measured on the CPU (tools/make_golden_q105.py asserts it):
#   mask on:  gain 1: r = 4.9e-4.
#   mask off: gain 1: r = 5.1e-2, 0.7: above 3.7e-2, 0.5: 3.7e-2, 0.35: 5.2e-3.  With the activation inside the blocks and pre-BatchNorm
#             variances far above eps = 1e-3 the f32 forward error grows ~2.3 x per block (1.8e-7 after first_cnn, 3.8e-4 after
#             last_cnn2, 192 activations on the other side of zero); at gain 0.35 the variances come down to the order of eps, the
#             growth stops (4.6e-6 after last_cnn2, 5 activations flipped).
GOLDEN_GAIN = {True: 1.0, False: 0.35}


def block_table() -> List[Tuple[str, int, int, int]]:
    return list(BLOCKS)


def unit_table() -> List[Tuple[str, str, int, int, int]]:
    """[(unit name of the plan, state-dict prefix of its SeprationConv, ci, co, k)] for the 50 block sub-units, in forward order"""
    out = []
    for name, ci, co, k in BLOCKS:
        for s in range(REPEAT - 1):
            out.append(("%s.seq.%d" % (name, s), "encoder.%s.seq.%d" % (name, s), ci, ci, k))
        out.append((name, "encoder.%s.seq.%d" % (name, REPEAT - 1), ci, co, k))
    return out


def state_shapes(n_class: int, in_c: int = 64):
    """Ordered (key, shape) list == MyModel2(encoder=QuartNet105).state_dict(): per block reside.0, reside.1.*, seq.0 .. seq.4"""
    out = R._sep_shapes("encoder.first_cnn", in_c, 256, 33, False)
    for name, ci, co, k in BLOCKS:
        p = "encoder." + name
        out += [(p + ".reside.0.weight", (co, ci, 1))] + R._bn_shapes(p + ".reside.1", co)
        for s in range(REPEAT):
            out += R._sep_shapes("%s.seq.%d" % (p, s), ci, co if s == REPEAT - 1 else ci, k, False)
    out += [("encoder.last_cnn2.0.weight", (1024, 512, 1))] + R._bn_shapes("encoder.last_cnn2.1", 1024)
    out += [("decoder.weight", (n_class, 1024, 1)), ("decoder.bias", (n_class,))]
    return out


def _is_bn(key: str) -> bool:
    return ".bn." in key or ".reside.1." in key or ".last_cnn2.1." in key


def formula_state(n_class: int, in_c: int = 64, gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """R.formula_state's rules over this variant's layout: tensor #idx, element #i: a (2u - 1), u = R.hash_uniform(i, idx),
    a = gain / sqrt(fan_in); BN gamma = 1 + 0.1 (2u - 1), beta = 0.1 (2u - 1); running_mean 0, running_var 1."""
    sd: Dict[str, torch.Tensor] = {}
    for idx, (key, shape) in enumerate(state_shapes(n_class, in_c)):
        n = int(np.prod(shape)) if len(shape) else 1
        if key.endswith("num_batches_tracked"):
            t = torch.zeros((), dtype=torch.int64)
        elif key.endswith("running_mean"):
            t = torch.zeros(shape)
        elif key.endswith("running_var"):
            t = torch.ones(shape)
        else:
            u = torch.from_numpy(2.0 * R.hash_uniform(n, idx) - 1.0)
            if _is_bn(key):
                t = ((1.0 if key.endswith("weight") else 0.0) + 0.1 * u).float().reshape(shape)
            else:
                fan_in = 1024 if key == "decoder.bias" else int(np.prod(shape[1:]))
                t = (gain / math.sqrt(fan_in) * u).float().reshape(shape)
        sd[key] = t
    return sd


def random_state(n_class: int, seed: int = 0, in_c: int = 64) -> Dict[str, torch.Tensor]:
    """R.random_state's rules (PyTorch-default-like U(-1/sqrt(fan_in), ..), BN 1 / 0) over this variant's layout"""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for key, shape in state_shapes(n_class, in_c):
        if key.endswith("num_batches_tracked"):
            t = torch.zeros((), dtype=torch.int64)
        elif key.endswith("running_mean"):
            t = torch.zeros(shape)
        elif key.endswith("running_var"):
            t = torch.ones(shape)
        elif _is_bn(key):
            t = torch.ones(shape) if key.endswith("weight") else torch.zeros(shape)
        else:
            bound = 1.0 / math.sqrt(1024 if key == "decoder.bias" else int(np.prod(shape[1:])))
            t = (torch.rand(shape, generator=g) * 2 - 1) * bound
        sd[key] = t
    return sd


class _Q105Blocks:
    """The block of QuartNet105 over the base oracle's own ``_sep`` / ``_bn`` / activation (mixed into both oracles below).
    The base classes are built as their "plain" variant (no SE, no context branch); only the block and the block loop differ."""

    def _sep_masked(self, x, lens, prefix: str, k: int, last: bool, mask: bool):
        saved = self.mask
        self.mask = mask
        try:
            return self._sep(x, lens, prefix, k, 1, last)
        finally:
            self.mask = saved

    def _inner(self, x, lens, prefix: str, k: int):
        """seq.0 .. seq.3: last = the model's mask, the sub-block's own mask = True (the quirk)"""
        return self._sep_masked(x, lens, prefix, k, last=bool(self.mask), mask=True)

    def _closing(self, x, x_block, lens, name: str, k: int):
        """seq.4 (last=True, mask = the model's) + reside(block input) + last_relu"""
        p = "encoder." + name
        main = self._sep_masked(x, lens, "%s.seq.%d" % (p, REPEAT - 1), k, last=True, mask=bool(self.mask))
        res = self._bn(F.conv1d(x_block, self.state[p + ".reside.0.weight"]), p + ".reside.1")
        return R.activation(main + res, self.act)

    def _block(self, x, lens, name: str, k: int):
        start = x
        for s in range(REPEAT - 1):
            x = self._inner(x, lens, "encoder.%s.seq.%d" % (name, s), k)
            if self.keep_taps:
                self.taps["%s.seq.%d" % (name, s)] = x
        return self._closing(x, start, lens, name, k)

    def _blocks(self, x, lens):
        for name, ci, co, k in BLOCKS:
            x = self._block(x, lens, name, k)
            if self.keep_taps:
                self.taps[name] = x
        return x


class OracleModel(_Q105Blocks, R.OracleModel):
    """R.OracleModel (the pinned f32 restatement; also runs in f64 when the state and the inputs are f64) with QuartNet105's blocks"""

    def __init__(self, n_class: int, mask: bool = True, act: str = "relu", state: Optional[Dict[str, torch.Tensor]] = None,
                 in_c: int = 64):
        R.OracleModel.__init__(self, "plain", n_class, mask, act, state if state is not None else random_state(n_class, 0, in_c), in_c)

    def encode(self, inputs, pct):
        x = inputs.squeeze(1)
        T1 = (x.size(2) + 2 * 16 - 33) // 2 + 1
        lens = R.mask_lengths(T1, pct)
        x = self._sep(x, lens, "encoder.first_cnn", 33, 2, False)
        if self.keep_taps:
            self.taps["first_cnn"] = x
        x = self._blocks(x, lens)
        y = F.conv1d(x, self.state["encoder.last_cnn2.0.weight"])
        x = R.activation(self._bn(y, "encoder.last_cnn2.1"), self.act)
        if self.keep_taps:
            self.taps["last_cnn2"] = x
        return x

    def forward(self, inputs, pct):
        x = self.encode(inputs, pct)
        logits = F.conv1d(x, self.state["decoder.weight"], self.state["decoder.bias"])
        return F.log_softmax(logits.transpose(1, 2), dim=-1)

    __call__ = forward


def cast_state(state: Dict[str, torch.Tensor], dtype) -> Dict[str, torch.Tensor]:
    return {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in state.items()}


class Bf16OracleModel(_Q105Blocks, E.Bf16OracleModel):
    """E.Bf16OracleModel (bf16 storage points, arithmetic in ``dtype`` between them; emulate=False: the plain oracle in ``dtype``)
    with QuartNet105's blocks"""

    def __init__(self, n_class: int, mask: bool = True, act: str = "relu", state: Optional[Dict[str, torch.Tensor]] = None,
                 in_c: int = 64, dtype=torch.float64, emulate: bool = True):
        E.Bf16OracleModel.__init__(self, "plain", n_class, mask, act, state if state is not None else random_state(n_class, 0, in_c),
                                   in_c, dtype, emulate)

    def _inner(self, x, lens, prefix: str, k: int):
        last = bool(self.mask)
        z = self._sep_masked(x, lens, prefix, k, last=last, mask=True)
        return self.st(z) if last else z          # (E._sep stores the output itself when the unit has its activation)

    def _closing(self, x, x_block, lens, name: str, k: int):
        p = "encoder." + name
        main = self._sep_masked(x, lens, "%s.seq.%d" % (p, REPEAT - 1), k, last=True, mask=bool(self.mask))
        y2 = self.st(F.conv1d(self.gs(x_block), self.sh(self.state[p + ".reside.0.weight"])))      # dx_res is its own bf16 tensor
        if self.keep_taps:
            self.taps[p + ".y2"] = y2
        res = self._bn(y2, p + ".reside.1")
        return self.st(self._act(main + res))

    def encode(self, inputs, pct):
        x = inputs.to(self.dtype).squeeze(1)
        if self.emulate:
            x = E.rb(x)
        T1 = (x.size(2) + 2 * 16 - 33) // 2 + 1
        lens = R.mask_lengths(T1, pct)
        x = self._sep(x, lens, "encoder.first_cnn", 33, 2, False)
        if self.keep_taps:
            self.taps["first_cnn"] = x
        x = self._blocks(x, lens)
        x = self._last(x)
        if self.keep_taps:
            self.taps["last_cnn2"] = x
        return x


def run_unit(model: Bf16OracleModel, unit: str, x_in: torch.Tensor, lens: torch.Tensor, dout: Optional[torch.Tensor],
             act_mask: Optional[torch.Tensor] = None, drop=None, x_block: Optional[torch.Tensor] = None):
    """One unit of the q105 plan from its own stored input(s), like E.run_unit: 'first_cnn', 'last_cnn2', an inner sub-unit
    '<block>.seq.<i>' or a closing sub-unit '<block>' (which also takes x_block, the block's input, for its residual branch).
    Returns {"u", "y", ["y2"], "out", "dx" (w.r.t. x_in, stored form), "dx_raw" (before the store), ["dx_res" (w.r.t. x_block, the
    bf16 tensor the plan keeps for the block's first sub-unit)], "grads"}."""
    model.training, model.keep_taps, model.taps = True, True, {}
    model.forced_mask = act_mask
    model.drop = drop
    units = {u[0]: u for u in unit_table()}
    if unit == "first_cnn":
        prefixes, pfx = ["encoder.first_cnn."], "encoder.first_cnn"
    elif unit == "last_cnn2":
        prefixes, pfx = ["encoder.last_cnn2."], "encoder.last_cnn2"
    else:
        _, pfx, ci, co, k = units[unit]
        prefixes = [pfx + "."] + (["encoder.%s.reside." % unit] if "." not in unit else [])
    params = {k_: v for k_, v in model.state.items() if not R.is_buffer(k_) and any(k_.startswith(p) for p in prefixes)}
    for p in params.values():
        p.requires_grad_(True)
        p.grad = None
    want = dout is not None
    x = x_in.to(model.dtype).detach().clone().requires_grad_(want and unit != "first_cnn")
    xb = None
    if unit == "first_cnn":
        out = model._sep(x, lens, pfx, 33, 2, False)
    elif unit == "last_cnn2":
        out = model._last(x)
    elif "." in unit:
        out = model._inner(x, lens, pfx, k)
    else:
        xb = x_block.to(model.dtype).detach().clone().requires_grad_(want)
        out = model._closing(x, xb, lens, unit, k)
    res = {"out": out.detach()}
    for name, key in (("u", pfx + ".u"), ("y", pfx + ".y"), ("y2", "encoder." + unit + ".y2")):
        if key in model.taps:
            res[name] = model.taps[key].detach()
    if want:
        out.backward(dout.to(model.dtype))
        if x.grad is not None:
            res["dx_raw"] = x.grad.detach()
            res["dx"] = E.rb(x.grad) if model.emulate else x.grad.detach()
        if xb is not None:
            res["dx_res"] = xb.grad.detach()          # (already a bf16 value under emulation: model.gs rounds it)
        res["grads"] = {k_: p.grad.detach().clone() for k_, p in params.items()}
    for p in params.values():
        p.requires_grad_(False)
        p.grad = None
    model.keep_taps, model.taps, model.drop = False, {}, None
    model.forced_mask = None
    return res
