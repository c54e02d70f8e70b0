"""``Novograd`` with the reference's constructor (scheduler/novograd.py:49-73) as a torch Optimizer
whose step() is ONE multi-tensor HIP call over the model's flat parameter / gradient buffers
(csrc/optim.hip), instead of ~10 tiny kernels per tensor."""
from __future__ import annotations

import torch
from torch.optim.optimizer import Optimizer

from .. import ops


def check_ema_decay(decay) -> float:
    """``ema_decay``: a finite number in [0, 1); 0 = no weight EMA"""
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 <= float(decay) < 1.0):
        raise ValueError("ema_decay has to be a number in [0, 1) (0 = off), got %r" % (decay,))
    return float(decay)


def check_grad_clip(gradient_clip_val, gradient_clip_algorithm="norm"):
    """``gradient_clip_val``: a finite number >= 0 (0 or None = no clipping); ``gradient_clip_algorithm``: "norm" or "value".
    Returns (float value, algorithm); a bad one raises ValueError naming the argument."""
    import math
    v = 0.0 if gradient_clip_val is None else gradient_clip_val
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)) or float(v) < 0.0:
        raise ValueError("gradient_clip_val has to be a finite number >= 0 (0 = off), got %r" % (gradient_clip_val,))
    if gradient_clip_algorithm not in ("norm", "value"):
        raise ValueError("gradient_clip_algorithm has to be 'norm' or 'value', got %r" % (gradient_clip_algorithm,))
    return float(v), gradient_clip_algorithm


def make_clip_state(gradient_clip_val, gradient_clip_algorithm, skip_nonfinite, track_grad_norm, device, steps=0, skipped=0):
    """the device record of DESIGN 4, "Gradient clipping and the non-finite guard" for these settings - None when everything is off
    and the gradient norm is not asked for (the step then launches the kernels it always launched)"""
    if not (gradient_clip_val > 0.0 or skip_nonfinite or track_grad_norm):
        return None
    return ops.clip_state(gradient_clip_algorithm if gradient_clip_val > 0.0 else "off", gradient_clip_val, skip_nonfinite, steps, skipped,
                          device=device)


class Novograd(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.95, 0.98), eps=1e-8, weight_decay=0, grad_averaging=False,
                 amsgrad=False, luc=False, luc_trust=1e-3, luc_eps=1e-8, ema_decay: float = 0.0, ema_warmup: bool = True,
                 gradient_clip_val: float = 0.0, gradient_clip_algorithm: str = "norm", skip_nonfinite: bool = False,
                 track_grad_norm: bool = False):
        """ema_decay > 0: the optimiser also owns ``ema``, an exponential moving average of the parameters ("Weight EMA"),
        and its device record ``ema_state``; every ``step()`` - and every fused step that adopted this optimiser's state -
        updates it inside the update kernel.  0 (the default) = off: no buffer is allocated.
        gradient_clip_val > 0 (by global norm or by value), skip_nonfinite (a step whose gradient holds a NaN or an Inf updates
        nothing) and track_grad_norm (record the global gradient norm only): the optimiser owns the device record ``clip_state``
        the step's kernels decide by ("Gradient clipping and the non-finite guard").  All off (the default): no record."""
        ema_decay = check_ema_decay(ema_decay)
        gradient_clip_val, gradient_clip_algorithm = check_grad_clip(gradient_clip_val, gradient_clip_algorithm)
        if lr < 0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Betas have to be between 0 and 1: {betas}")
        if grad_averaging or amsgrad or luc:
            raise NotImplementedError("grad_averaging / amsgrad / luc are not used by the reference path (train.py:46) "
                                      "and are not implemented in the HIP kernel")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_averaging=False, amsgrad=False)
        super().__init__(params, defaults)
        owners = {id(getattr(p, "_lasr_owner", None)): getattr(p, "_lasr_owner", None)
                  for g in self.param_groups for p in g["params"]}
        if len(owners) != 1 or None in owners.values():
            raise ValueError("Novograd (HIP) optimises the parameters of exactly one MyModel2 (its flat GPU buffer)")
        self.owner = next(iter(owners.values()))
        n = self.owner.native
        if sum(len(g["params"]) for g in self.param_groups) != len(n.param_infos()):
            raise ValueError("Novograd (HIP) needs all parameters of the model in its param groups")
        self.exp_avg = torch.zeros_like(n.params)
        self.exp_avg_sq = torch.zeros(len(n.param_infos()), dtype=torch.float32, device=n.device)
        self.offsets = n.param_offsets()
        self.lr_dev = torch.zeros(1, dtype=torch.float32, device=n.device)
        self.grad_scale = 1.0          # set to 1/world by the data-parallel wrapper after a SUM all-reduce
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.ema = self.ema_state = None
        if ema_decay > 0.0:            # the average starts as a copy of the parameters at the moment it is switched on
            self.ema = n.params.clone()
            self.ema_state = ops.ema_state(ema_decay, self.ema_warmup, 0, device=n.device)
        self.gradient_clip_val, self.gradient_clip_algorithm = gradient_clip_val, gradient_clip_algorithm
        self.skip_nonfinite, self.track_grad_norm = bool(skip_nonfinite), bool(track_grad_norm)
        self.clip_state = make_clip_state(gradient_clip_val, gradient_clip_algorithm, self.skip_nonfinite, self.track_grad_norm, n.device)

    @property
    def skipped_steps(self) -> int:
        """optimiser steps dropped as non-finite so far (one read of the device record); 0 without a record"""
        return ops.clip_state_read(self.clip_state)["skipped"] if self.clip_state is not None else 0

    @property
    def ema_num_updates(self) -> int:
        """EMA updates done so far (one read of the device record); 0 with EMA off"""
        return ops.ema_state_read(self.ema_state)["num_updates"] if self.ema_state is not None else 0

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        n = self.owner.native
        self.lr_dev.fill_(float(g["lr"]))
        ops.novograd_step(n.params, n.grads, self.exp_avg, self.exp_avg_sq, self.offsets, self.lr_dev, g["betas"][0],
                          g["betas"][1], g["eps"], g["weight_decay"], self.grad_scale, ema=self.ema, ema_state=self.ema_state,
                          clip_state=self.clip_state)
        return loss

    def zero_grad(self, set_to_none: bool = True):
        # gradients live in the flat buffer: the first backward after this overwrites it whole, further ones add (models/_base.py)
        for g in self.param_groups:
            for p in g["params"]:
                p.grad = None

    def state_dict(self):
        sd = super().state_dict()
        sd["lasr"] = {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone()}
        if self.ema is not None:
            sd["lasr"].update(ema=self.ema.clone(), ema_num_updates=self.ema_num_updates, ema_decay=self.ema_decay,
                              ema_warmup=self.ema_warmup)
        if self.clip_state is not None:
            st = ops.clip_state_read(self.clip_state)
            sd["lasr"].update(clip_steps=st["steps"], clip_skipped=st["skipped"])
        return sd

    def load_state_dict(self, sd):
        extra = sd.pop("lasr", None)
        super().load_state_dict(sd)
        if extra is not None:
            self.exp_avg.copy_(extra["exp_avg"])
            self.exp_avg_sq.copy_(extra["exp_avg_sq"])
        if self.ema is not None:
            # the decay and the warm-up flag are this optimiser's own (the run's configuration); the average and its count are the
            # checkpoint's.  A state without them (an EMA-less run resumed with EMA on): the average restarts from the parameters
            # as they are now - the caller loads the model first (Trainer.fit does)
            if extra is not None and extra.get("ema") is not None:
                self.ema.copy_(extra["ema"])
                count = int(extra.get("ema_num_updates", 0))
            else:
                self.ema.copy_(self.owner.native.params)
                count = 0
            self.ema_state.copy_(ops.ema_state(self.ema_decay, self.ema_warmup, count, device=self.ema_state.device))
        if self.clip_state is not None:
            # the mode, the value and the guard are this run's configuration; the two counts are the checkpoint's (0 without them)
            got = extra or {}
            self.clip_state.copy_(make_clip_state(self.gradient_clip_val, self.gradient_clip_algorithm, self.skip_nonfinite,
                                                  self.track_grad_norm, self.clip_state.device, int(got.get("clip_steps", 0)),
                                                  int(got.get("clip_skipped", 0))))
