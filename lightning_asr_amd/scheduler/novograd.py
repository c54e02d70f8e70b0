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


STATE_NAMES = ("exp_avg", "exp_avg_sq", "offsets", "lr_dev", "ema", "ema_state", "clip_state", "ema_decay", "ema_warmup",
               "gradient_clip_val", "gradient_clip_algorithm", "skip_nonfinite", "track_grad_norm", "ema_num_updates", "skipped_steps")


def forwards_opt_state(cls):
    """class decorator: the names of the ``OptimState`` an instance holds as ``opt_state`` read through on the instance itself"""
    for name in STATE_NAMES:
        setattr(cls, name, property(lambda self, _n=name: getattr(self.opt_state, _n)))
    return cls


class OptimState:
    """The optimiser's device state and the settings its kernels decide by, in ONE place: the NovoGrad moments, the device
    learning rate, the weight EMA with its record, the clip record and the kept workspace.  ``Novograd`` holds one; a ``TrainStep``
    holds its own or, built by ``from_optimizer``, the optimiser's - so the fused route trains the very tensors checkpoints save."""

    def __init__(self, ema_decay: float = 0.0, ema_warmup: bool = True, gradient_clip_val: float = 0.0,
                 gradient_clip_algorithm: str = "norm", skip_nonfinite: bool = False, track_grad_norm: bool = False):
        """Checks and keeps the settings; ``allocate`` makes the tensors (a bad setting is refused before any model is looked at).
        ema_decay > 0: ``ema`` is an exponential moving average of the parameters ("Weight EMA"), updated by the last kernel
        of every optimiser step with the weight the device record ``ema_state`` yields - no launch, no host scalar, so a captured
        graph replays it.  0 = off: no buffer, and the step as it always was.
        gradient_clip_val > 0 / gradient_clip_algorithm ("norm": by the global norm, "value": element-wise) / skip_nonfinite (a step
        whose gradient holds a NaN or an Inf leaves parameters, moments and the average alone, and still counts as a step) /
        track_grad_norm (record the global norm only): decided on the device by the optimiser's own kernels through the record
        ``clip_state`` ("Gradient clipping and the non-finite guard") - no launch, no host decision.  All off: no record."""
        self.ema_decay, self.ema_warmup = check_ema_decay(ema_decay), bool(ema_warmup)
        self.gradient_clip_val, self.gradient_clip_algorithm = check_grad_clip(gradient_clip_val, gradient_clip_algorithm)
        self.skip_nonfinite, self.track_grad_norm = bool(skip_nonfinite), bool(track_grad_norm)

    def allocate(self, native, lr: float = 0.0) -> "OptimState":
        """the state for ``native``'s flat parameters: zero moments, the average (a copy of the parameters as they are now) and the
        clip record - the latter two None when switched off: no buffer, no record"""
        dev = native.device
        self.exp_avg = torch.zeros_like(native.params)
        self.exp_avg_sq = torch.zeros(len(native.param_infos()), dtype=torch.float32, device=dev)
        self.offsets = native.param_offsets()
        self.lr_dev = torch.tensor([float(lr)], dtype=torch.float32, device=dev)
        self.ema = self.ema_state = None
        if self.ema_decay > 0.0:
            self.ema = native.params.clone()
            self.ema_state = ops.ema_state(self.ema_decay, self.ema_warmup, 0, device=dev)
        self.clip_state = self._clip_record(dev)
        self._opt_ws = None            # kept across steps: zeroed once, left zeroed by every step (no memset launch)
        return self

    def _clip_record(self, device, steps=0, skipped=0):
        """the device record of DESIGN 4, "Gradient clipping and the non-finite guard" for the settings - None when everything is off
        and the gradient norm is not asked for (the step then launches the kernels it always launched)"""
        if not (self.gradient_clip_val > 0.0 or self.skip_nonfinite or self.track_grad_norm):
            return None
        return ops.clip_state(self.gradient_clip_algorithm if self.gradient_clip_val > 0.0 else "off", self.gradient_clip_val,
                              self.skip_nonfinite, steps, skipped, device=device)

    @property
    def ema_num_updates(self) -> int:
        """EMA updates done so far (one read of the device record); 0 with EMA off"""
        return ops.ema_state_read(self.ema_state)["num_updates"] if self.ema_state is not None else 0

    @property
    def skipped_steps(self) -> int:
        """optimiser steps dropped as non-finite so far (one read of the device record); 0 without a record"""
        return ops.clip_state_read(self.clip_state)["skipped"] if self.clip_state is not None else 0

    def step(self, params, grads, betas, eps, weight_decay, grad_scale) -> None:
        """the one NovoGrad call, through the kept workspace (for ``Novograd.step`` too, which used to zero one of its own per call)"""
        if self._opt_ws is None:
            self._opt_ws = ops.novograd_workspace(self.exp_avg_sq.numel(), params.numel(), params.device)
        ops.novograd_step(params, grads, self.exp_avg, self.exp_avg_sq, self.offsets, self.lr_dev, betas[0], betas[1], eps, weight_decay,
                          grad_scale=grad_scale, ws=self._opt_ws, ema=self.ema, ema_state=self.ema_state, clip_state=self.clip_state)

    def tensors(self):
        """every device tensor a snapshot of the training state has to cover"""
        return [t for t in (self.exp_avg, self.exp_avg_sq, self.lr_dev, self.ema, self.ema_state, self.clip_state) if t is not None]

    def extra_state(self) -> dict:
        """the "lasr" part of the optimiser's state_dict"""
        extra = {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone()}
        if self.ema is not None:
            extra.update(ema=self.ema.clone(), ema_num_updates=self.ema_num_updates, ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)
        if self.clip_state is not None:
            st = ops.clip_state_read(self.clip_state)
            extra.update(clip_steps=st["steps"], clip_skipped=st["skipped"])
        return extra

    def load_extra_state(self, extra, live_params) -> None:
        """extra: a checkpoint's "lasr" part, or None.  The settings stay this run's; moments, average and counts are the checkpoint's."""
        if extra is not None:
            self.exp_avg.copy_(extra["exp_avg"])
            self.exp_avg_sq.copy_(extra["exp_avg_sq"])
        if self.ema is not None:
            # a state without an average (an EMA-less run resumed with EMA on): it restarts from the parameters as they are now -
            # the caller loads the model first (Trainer.fit does)
            if extra is not None and extra.get("ema") is not None:
                self.ema.copy_(extra["ema"])
                count = int(extra.get("ema_num_updates", 0))
            else:
                self.ema.copy_(live_params)
                count = 0
            self.ema_state.copy_(ops.ema_state(self.ema_decay, self.ema_warmup, count, device=self.ema_state.device))
        if self.clip_state is not None:
            got = extra or {}           # the two counts are 0 without them
            self.clip_state.copy_(self._clip_record(self.clip_state.device, int(got.get("clip_steps", 0)), int(got.get("clip_skipped", 0))))


@forwards_opt_state
class Novograd(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.95, 0.98), eps=1e-8, weight_decay=0, grad_averaging=False,
                 amsgrad=False, luc=False, luc_trust=1e-3, luc_eps=1e-8, ema_decay: float = 0.0, ema_warmup: bool = True,
                 gradient_clip_val: float = 0.0, gradient_clip_algorithm: str = "norm", skip_nonfinite: bool = False,
                 track_grad_norm: bool = False):
        """The device state is ``self.opt_state``, an ``OptimState`` whose names (``exp_avg``, ``ema``, ``clip_state`` ...) read through on
        the optimiser; the last six arguments are its settings.  Every ``step()`` - and every fused step over this state - uses it."""
        opt_state = OptimState(ema_decay, ema_warmup, gradient_clip_val, gradient_clip_algorithm, skip_nonfinite, track_grad_norm)
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
        self.opt_state = opt_state.allocate(n)
        self.grad_scale = 1.0          # set to 1/world by the data-parallel wrapper after a SUM all-reduce

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        n = self.owner.native
        self.lr_dev.fill_(float(g["lr"]))
        self.opt_state.step(n.params, n.grads, g["betas"], g["eps"], g["weight_decay"], self.grad_scale)
        return loss

    def zero_grad(self, set_to_none: bool = True):
        # gradients live in the flat buffer: the first backward after this overwrites it whole, further ones add (models/_base.py)
        for g in self.param_groups:
            for p in g["params"]:
                p.grad = None

    def state_dict(self):
        sd = super().state_dict()
        sd["lasr"] = self.opt_state.extra_state()
        return sd

    def load_state_dict(self, sd):
        extra = sd.pop("lasr", None)
        super().load_state_dict(sd)
        self.opt_state.load_extra_state(extra, self.owner.native.params)
