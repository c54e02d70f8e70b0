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


class Novograd(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.95, 0.98), eps=1e-8, weight_decay=0, grad_averaging=False,
                 amsgrad=False, luc=False, luc_trust=1e-3, luc_eps=1e-8, ema_decay: float = 0.0, ema_warmup: bool = True):
        """ema_decay > 0: the optimiser also owns ``ema``, an exponential moving average of the parameters ("Weight EMA"),
        and its device record ``ema_state``; every ``step()`` - and every fused step that adopted this optimiser's state -
        updates it inside the update kernel.  0 (the default) = off: no buffer is allocated."""
        ema_decay = check_ema_decay(ema_decay)
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
                          g["betas"][1], g["eps"], g["weight_decay"], self.grad_scale, ema=self.ema, ema_state=self.ema_state)
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
