"""One data-parallel training step of the hot path, entirely on the GPU:

    wave (HBM) -> log-mel features -> QuartzNet forward -> mean CTC -> backward
               -> gradient all-reduce (RCCL over xGMI, world > 1) -> NovoGrad -> LR schedule

This is what ``LightingModule.training_step`` + Lightning's optimiser loop do in the reference
(train.py:64-86, scheduler/novograd.py:75-145); here each stage is one or a few C-ABI calls."""
from __future__ import annotations

from typing import Optional

import torch

import contextlib
import ctypes as C
import os

from . import _lib, ops
from .comm import Communicator
from .engine import NativeModel
from .schedule import CosineAnnealingWarmupRestarts
from .scheduler.novograd import OptimState, forwards_opt_state


_ROCTX = None


def _roctx_on() -> bool:
    global _ROCTX
    if _ROCTX is None:
        _ROCTX = os.environ.get("LASR_ROCTX", "0") not in ("", "0") and bool(_lib.load().lasr_roctx_enabled())
    return _ROCTX


def check_accumulate(k) -> int:
    """``accumulate_grad_batches``: an int >= 1 (Lightning's epoch -> K dict is not implemented)"""
    if isinstance(k, dict):
        raise NotImplementedError("accumulate_grad_batches as a dict (epoch -> K) is not implemented: pass one int >= 1")
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("accumulate_grad_batches has to be an int >= 1, got %r" % (k,))
    return k


class _TorchDistExchange:
    """``Communicator``'s collectives over torch.distributed (gloo groups, ``LASR_COMM=torch``, the fall-back of the communicator's
    self-check): the bucket all-reduces are asynchronous and ``wait`` joins them; the flat all-reduce and the broadcast block"""

    def __init__(self, process_group):
        self.pg, self.works = process_group, []

    def all_reduce_ranges(self, flat, ranges) -> None:
        self.works.extend(torch.distributed.all_reduce(flat[lo:hi], group=self.pg, async_op=True) for lo, hi in ranges)

    def all_reduce(self, flat) -> None:
        torch.distributed.all_reduce(flat, group=self.pg)

    def broadcast(self, flat, root: int = 0) -> None:
        torch.distributed.broadcast(flat, root, group=self.pg)

    def wait(self) -> None:
        works, self.works = self.works, []
        for w in works:
            w.wait()


@forwards_opt_state
class TrainStep:
    def __init__(self, model: NativeModel, learning_rate: float = 1e-2, weight_decay: float = 1e-3,
                 betas=(0.8, 0.5), eps: float = 1e-8, schedule: Optional[CosineAnnealingWarmupRestarts] = None,
                 process_group=None, comm: Optional[Communicator] = None, accumulate: int = 1, ema_decay: float = 0.0,
                 ema_warmup: bool = True, gradient_clip_val: float = 0.0, gradient_clip_algorithm: str = "norm",
                 skip_nonfinite: bool = False, track_grad_norm: bool = False, opt_state: Optional[OptimState] = None):
        """comm: the library-owned RCCL communicator (lasr_comm_*).  Default for world > 1 on the nccl backend: one is built
        from the torch.distributed group (which then only bootstraps the unique id); ``LASR_COMM=torch`` keeps the gradient
        exchange on torch.distributed (the only choice for gloo groups: CPU rehearsal, two ranks sharing a GPU in the tests).
        accumulate: K = ``accumulate_grad_batches``.  K > 1: every call is one MICRO-step (forward, loss, backward into
        ``model.grads_micro``, one launch that adds it into ``model.grads``); the K-th of a window - or one called with
        ``last=True`` - is the boundary, which additionally all-reduces, steps the optimiser with grad_scale 1 / (K world),
        steps the schedule and zeroes ``model.grads``, which is therefore zero between windows.  K = 1 is the step as it
        always was: no second buffer, no extra launch.
        opt_state: the optimiser's device state (moments, learning rate, weight EMA, clip record) as ONE ``OptimState``, whose names
        read through on the step (``self.ema``, ``self.clip_state``, ``self.skipped_steps`` ...): the one handed in (``from_optimizer``)
        or, by default, its own, made from the six settings before it (``OptimState.__init__``).  Under accumulate > 1 only the
        boundary reaches the EMA update, and clipping and the non-finite guard act once per window, on the window's sum."""
        self.model = model
        self.schedule = schedule
        self.lr = schedule.lr if schedule is not None else learning_rate
        settings = (ema_decay, ema_warmup, gradient_clip_val, gradient_clip_algorithm, skip_nonfinite, track_grad_norm)
        if opt_state is not None and settings != (0.0, True, 0.0, "norm", False, False):
            raise ValueError("opt_state carries its own settings: ema_decay ... track_grad_norm cannot be passed beside it")
        self.opt_state = opt_state if opt_state is not None else OptimState(*settings).allocate(model, self.lr)
        self.accumulate = check_accumulate(accumulate)
        self.micro = 0             # micro-batches already added into model.grads in the current window (K > 1)
        if self.accumulate > 1:
            model.grads.zero_()
        self.wd, self.betas, self.eps = weight_decay, betas, eps
        self.pg = process_group
        self.world = 1
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
        self.global_step = 0
        self.overlap = True        # overlap the gradient all-reduce with backward (world > 1)
        self.comm = comm
        if comm is not None:
            self.world = comm.world
        elif self.world > 1 and os.environ.get("LASR_COMM", "rccl") == "rccl" and \
                (torch.distributed.get_backend(process_group) == "nccl" or os.environ.get("LASR_RCCL_PATH")):   # (gloo + LASR_RCCL_PATH: rehearsal over the test stub)
            self.comm = self._checked_communicator(model.device, process_group)
        # how gradients and parameters travel between the ranks, chosen once (at world 1 without a communicator: nothing calls it)
        self._exchange = self.comm if self.comm is not None else _TorchDistExchange(process_group)
        # exercise the staged + async all-reduce path on a 1-rank group too (validation on one GPU)
        self.force_staged = bool(int(os.environ.get("LASR_FORCE_OVERLAP", "0"))) and \
            (self.comm is not None or torch.distributed.is_initialized())
        self._prefetched = None    # (key, feats, pct) of the batch announced by the previous step(prefetch_wave=...)
        self._lr_state = None      # device image of the schedule (use_device_schedule)
        self._lr_epoch = None      # host schedule position the device image corresponds to

    @staticmethod
    def _checked_communicator(dev, process_group) -> Optional[Communicator]:
        """The library's RCCL communicator, proven on THIS machine before it carries gradients: every rank all-reduces
        (rank + 1, 1) through it on the side stream and must read (world (world + 1) / 2, world); the ranks then agree (one
        torch.distributed MIN) on whether all of them passed.  Any failure - librccl missing, init error, a wrong sum - sends the
        whole group back to torch.distributed's all-reduce (what LASR_COMM=torch selects), loudly."""
        import sys
        import torch.distributed as dist
        comm, ok, why = None, 1, ""
        try:
            comm = Communicator.from_torch_distributed(dev, process_group)
            probe = torch.tensor([float(comm.rank + 1), 1.0], dtype=torch.float32, device=dev)
            comm.all_reduce(probe)
            comm.wait()
            w = comm.world
            got = probe.cpu().tolist()
            if got != [w * (w + 1) / 2.0, float(w)]:
                ok, why = 0, "all-reduce self-check read %s" % (got,)
        except Exception as e:  # noqa: BLE001
            ok, why = 0, "%s: %s" % (type(e).__name__, e)
        flag = torch.tensor([ok], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=process_group)
        if int(flag.item()) == 1:
            return comm
        sys.stderr.write("lasr_comm self-check failed on rank %d (%s): gradient exchange falls back to torch.distributed\n"
                         % (dist.get_rank(process_group), why or "another rank failed"))
        if comm is not None:
            comm.close()
        return None

    @classmethod
    def from_optimizer(cls, model: NativeModel, optimizer, schedule=None, process_group=None, comm: Optional[Communicator] = None,
                       accumulate: int = 1):
        """The fused step over the state of a ``scheduler.novograd.Novograd`` (+ its ``CosineAnnealingWarmupRestarts``): the step's
        ``opt_state`` IS the optimizer's - moments, device learning rate, weight EMA, clip record - so ``optimizer.state_dict()`` /
        checkpoints / resume keep working while ``Trainer.fit`` drives this step instead of ``loss.backward(); optimizer.step()``."""
        g = optimizer.param_groups[0]
        ts = cls(model, learning_rate=float(g["lr"]), weight_decay=g["weight_decay"], betas=tuple(g["betas"]), eps=g["eps"],
                 schedule=schedule, process_group=process_group, comm=comm, accumulate=accumulate, opt_state=optimizer.opt_state)
        ts.lr = float(g["lr"])
        ts.lr_dev.fill_(ts.lr)
        return ts

    def sync_device_schedule(self) -> None:
        """Re-upload the schedule after its host state changed behind the device twin's back (``load_state_dict`` on resume,
        an assignment to ``ts.lr``): the rate the optimiser reads and the device state restart from the host object."""
        if self.schedule is not None:
            self.lr = self.schedule.lr
        self.lr_dev.fill_(float(self.lr))
        if self._lr_state is not None:         # in place: a captured graph holds the address of the device state
            self._lr_state.copy_(self._schedule_image())
            self._lr_epoch = int(self.schedule.last_epoch)

    def broadcast_parameters(self, src: int = 0) -> None:
        """DDP wrap-time broadcast of parameters and buffers from rank 0 (a one-rank communicator still runs its own)."""
        if self.comm is not None or self.world > 1:
            self._exchange.broadcast(self.model.params, src)
            self._exchange.broadcast(self.model.buffers, src)
            self._exchange.wait()

    def features(self, wave, sample_lens=None, dither=None, aug=None, logical_len=None):
        """wave (B, L) f32 on the GPU -> ([B][T][64] features in the activation dtype, pct (B)).  logical_len: the longest utterance
        when the rows are wider than that (ops.mel)."""
        _, btf, _, pct = ops.mel(wave, sample_lens, dither, aug, True, self.model.act_dtype, want_bft=False, want_btf=True,
                                 logical_len=logical_len)
        return btf, pct

    def optimizer_step(self, reduced: bool = False) -> None:
        """reduced: the step body has already exchanged the gradient bucket by bucket; otherwise, at world > 1, one flat 20 MB SUM
        all-reduce here.  The 1/world average is folded into the optimiser's grad scale.  An optimiser step closes the accumulation
        window: called on its own in the middle of one (accumulate > 1), it resets ``self.micro`` too."""
        m = self.model
        if self.world > 1 and not reduced:
            self._exchange.all_reduce(m.grads)
            self._exchange.wait()
        self.opt_state.step(m.params, m.grads, self.betas, self.eps, self.wd, 1.0 / (self.accumulate * self.world))
        self.count_optimizer_step(advance_device=True)

    def count_optimizer_step(self, advance_device: bool) -> None:
        """Host bookkeeping after an optimiser step, eager or replayed: the host copy of the schedule (logging / checkpoints),
        ``global_step``, the window counter.  advance_device: the rate the next step reads is still to be advanced (not after a replay)."""
        if self.schedule is not None:
            if self._lr_state is not None and self.schedule.last_epoch != self._lr_epoch:
                self.sync_device_schedule()                # the host schedule was loaded / reset since the last step: the device
                advance_device = True                      # twin restarts (in place) at the host's position and advances with it
            self.lr = self.schedule.step()
            self._lr_epoch = self.schedule.last_epoch
            if advance_device and self._lr_state is not None:      # the rate the next step uses is computed on the device
                _lib.call("lasr_lr_schedule_step", self._lr_state.data_ptr(), self.lr_dev.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
            elif advance_device:
                self.lr_dev.fill_(self.lr)
        self.global_step += 1
        self.micro = 0

    @contextlib.contextmanager
    def preserved(self, extra=()):
        """Everything a training step changes - parameters, BN buffers and counters, the optimiser's state, the gradient sum and the
        micro-batch buffer (accumulate > 1), the schedule on both sides, the dropout counter, the step / window counters - plus the
        tensors in ``extra``: snapshotted on entry, put back on exit, also when the block raises.  No prefetch stays armed."""
        m = self.model
        tensors = [m.params, m.buffers] + self.opt_state.tensors() + ([m.grads, m.grads_micro] if self.accumulate > 1 else []) + \
            [t for t in (self._lr_state, getattr(m, "drop_step", None)) if t is not None] + list(extra)
        snap = [t.clone() for t in tensors]
        sched_sd = dict(self.schedule.state_dict()) if self.schedule is not None else None
        host = (self.global_step, self.micro, self._lr_epoch, m._bump)
        counters = {k: v.clone() for k, v in m.counters.items()}
        try:
            yield
        finally:
            torch.cuda.synchronize()
            for t, s_ in zip(tensors, snap):
                t.copy_(s_)
            if sched_sd is not None:
                self.schedule.load_state_dict(sched_sd)
                self.lr = self.schedule.lr
                self.schedule._publish()
            self.global_step, self.micro, self._lr_epoch, m._bump = host
            m.counters.update(counters)
            self._prefetched = None
            m.disarm_prefetch()
            torch.cuda.synchronize()

    def use_device_schedule(self) -> None:
        """Move the LR schedule's state onto the GPU (csrc/sched.hip): from now on every optimizer_step advances it with a
        one-thread kernel instead of a host scalar + fill, so the whole step is capturable.  The host object keeps stepping
        alongside (same values to f32 rounding) for logging and checkpoints."""
        if self.schedule is None or self._lr_state is not None:
            return
        self._lr_state = self._schedule_image().to(self.model.device)
        self._lr_epoch = int(self.schedule.last_epoch)

    def _schedule_image(self) -> torch.Tensor:
        """the host schedule as it stands, as the bytes of the device state"""
        sc = self.schedule
        nb = int(_lib.load().lasr_lr_schedule_state_bytes())
        host = C.create_string_buffer(nb)
        _lib.call("lasr_lr_schedule_init", host, nb, int(sc.first_cycle_steps), float(sc.cycle_mult), float(sc.base_max_lr),
                  float(sc.min_lr), int(sc.warmup_steps), float(sc.gamma), int(sc.cycle), int(sc.step_in_cycle),
                  int(sc.cur_cycle_steps), int(sc.last_epoch))
        return torch.frombuffer(bytearray(host.raw), dtype=torch.uint8)

    def step_features(self, feats, pct, targets, tgt_lens, want_logp: bool = True, last: Optional[bool] = None,
                      role: Optional[str] = None):
        """last (accumulate > 1): None - the boundary follows the window counter ``self.micro``; True - this micro-batch closes
        the window whatever it holds (the flush at the end of an epoch).  role: "accumulate" / "boundary" fixes the role
        outright (a captured graph holds one role).  Both are ignored at accumulate = 1."""
        boundary = True
        if self.accumulate > 1:
            if role not in (None, "accumulate", "boundary"):
                raise ValueError("role has to be 'accumulate' or 'boundary', got %r" % (role,))
            boundary = (role == "boundary") if role is not None else (bool(last) or self.micro + 1 >= self.accumulate)
        args = (feats, pct, targets, tgt_lens, want_logp, boundary)
        if _roctx_on():                      # LASR_ROCTX=1: "lasr:step" around the whole step (rocprofv3 --marker-trace)
            _lib.load().lasr_roctx_range_push(b"lasr:step")
            try:
                return self._step_body(*args)
            finally:
                _lib.load().lasr_roctx_range_pop()
        return self._step_body(*args)

    def _step_body(self, feats, pct, targets, tgt_lens, want_logp: bool, boundary: bool):
        """Backward, gradient exchange, optimiser step.  accumulate > 1 - one micro-step of a window, in two uniform roles: every
        micro-step ADDS its gradient to ``model.grads`` (zero at the start of a window), the boundary also exchanges, steps and
        zeroes - so a batch shape needs two captured graphs, not the three of "the first micro-batch overwrites".  accumulate = 1:
        always the boundary, straight into ``model.grads`` - no second buffer, no add, no zeroing."""
        m = self.model
        gm = m.grads_micro if self.accumulate > 1 else None
        staged = self.overlap and (self.world > 1 or self.force_staged)
        if staged:
            # data parallel: bucketed SUM all-reduce, launched bucket by bucket in reverse layer order while the units below are
            # still being differentiated (it waits only for the kernels enqueued so far; the optimiser waits for all buckets).
            # EVERY micro-step of a window takes this staged backward (the same kernels in the same split-K order throughout) and
            # adds each bucket into the running sum as soon as its stage is enqueued; only the boundary hands it to the all-reduce
            # right behind that add - the other micro-steps issue no collective (Lightning's no_sync)
            def on_bucket(ranges):
                if gm is not None:
                    ops.grad_accumulate(m.grads, gm, ranges)
                if boundary:
                    self._exchange.all_reduce_ranges(m.grads, ranges)
            out = m.loss_backward_staged(feats, pct, targets, tgt_lens, on_bucket, want_logp=want_logp, grads=gm)
            if boundary:
                self._exchange.wait()
        else:
            out = m.loss_backward(feats, pct, targets, tgt_lens, want_logp=want_logp, grads=gm)
            if gm is not None:
                ops.grad_accumulate(m.grads, gm)
        if boundary:
            self.optimizer_step(reduced=staged)    # (world > 1 and not staged: its one flat all-reduce, on the boundary only)
            if gm is not None:
                m.grads.zero_()
        else:
            self.micro += 1
        return out

    @staticmethod
    def _prefetch_key(wave, sample_lens, dither, aug):
        return tuple(None if t is None else ((t.data_ptr(), tuple(t.shape), t._version) if torch.is_tensor(t) else ("obj", id(t)))
                     for t in (wave, sample_lens, dither, aug))

    def step(self, wave, targets, tgt_lens, sample_lens=None, dither=None, aug=None, prefetch_wave=None, prefetch_lens=None,
             prefetch_dither=None, prefetch_aug=None, want_logp: bool = True, logical_len=None, prefetch_logical_len=None,
             last: Optional[bool] = None):
        """One training step on `wave` (accumulate > 1: one micro-step; ``last`` as in ``step_features``).  prefetch_wave: the NEXT step's waveforms (already in HBM): their log-mel features are
        computed during this step in the grid of the CTC lattice kernel (32 busy workgroups, 224 idle CUs for ~0.1 ms) and
        picked up by the next call if it passes the same tensors - the data-loader prefetch of the reference's workers;
        every step still computes exactly one batch of features."""
        pf, self._prefetched = self._prefetched, None
        if pf is not None and pf[0] == self._prefetch_key(wave, sample_lens, dither, aug):
            feats, pct = pf[1], pf[2]
        else:
            feats, pct = self.features(wave, sample_lens, dither, aug, logical_len=logical_len)
        nxt = None
        if prefetch_wave is not None:
            nf, npct = self.model.arm_prefetch(prefetch_wave, prefetch_lens, prefetch_dither, prefetch_aug, logical_len=prefetch_logical_len)
            nxt = (self._prefetch_key(prefetch_wave, prefetch_lens, prefetch_dither, prefetch_aug), nf, npct)
        out = self.step_features(feats, pct, targets, tgt_lens, want_logp=want_logp, last=last)
        self._prefetched = nxt
        return out


class GraphedTrainStep:
    """One static-shape training step captured into a hipGraph (torch.cuda.CUDAGraph over the stream the C ABI launches on) and
    replayed: ~200 kernel launches per step become one graph launch, so the step no longer depends on how fast the host can
    enqueue (measured on a box whose CPUs were shared with three other jobs: 2.9 ms/step host-bound against 2.35 ms of GPU work).

    ``step(next_wave, targets, tgt_lens)``: like the prefetching ``TrainStep.step`` - the replay trains on the features the
    PREVIOUS replay computed and computes the features of ``next_wave`` inside its CTC launch; ``targets`` belong to the batch
    being trained on.  prefetch=False: features and training step of the same ``wave`` in one replay.
    Shapes are fixed at construction; one instance per (B, L, S) - and, over a ``TrainStep(accumulate > 1)``, per role: a graph
    holds either the accumulate micro-step or the boundary micro-step (``role``; ignored at accumulate = 1)."""

    def __init__(self, ts: TrainStep, B: int, L: int, S: int, ragged: bool = False, prefetch: bool = True, want_logp: bool = False,
                 inputs=None, feats_in=None, feats_out=None, wave_dtype=torch.float32, with_aug: bool = False, dither=None,
                 logical_len: Optional[int] = None, role: str = "boundary"):
        """inputs = (wave, sample_lens | None, targets, tgt_lens[, aug]): tensors already resident in HBM that the graph reads IN
        PLACE (``replay()`` then takes no data and nothing is copied); otherwise static buffers are allocated and ``step()``
        copies into them.  feats_in / feats_out = (feats, pct) pairs: the features this graph trains on and where it writes the
        prefetched ones - two graphs with the pairs swapped ping-pong without the end-of-step copy.
        wave_dtype: torch.float32 or torch.int16 (PCM); with_aug: a static (B, 4) SpecAugment block; dither: None, a static
        (B, L) noise tensor or an ``ops.DeviceDither`` (fresh noise per replay)."""
        self.ts, self.prefetch, self.want_logp = ts, prefetch, want_logp
        if role not in ("accumulate", "boundary"):
            raise ValueError("role has to be 'accumulate' or 'boundary', got %r" % (role,))
        self.role = role if ts.accumulate > 1 else "boundary"
        self.logical_len = logical_len        # rows of L samples whose longest utterance has logical_len <= L (ops.mel): T follows it
        dev = ts.model.device
        self.bound = inputs is not None
        self.dither = dither
        if self.bound:
            self.wave, self.lens, self.targets, self.tgt_lens = inputs[:4]
            self.aug = inputs[4] if len(inputs) > 4 else None
        else:
            self.wave = torch.zeros(B, L, dtype=wave_dtype, device=dev)
            self.lens = torch.full((B,), L, dtype=torch.int32, device=dev) if ragged else None
            self.targets = torch.zeros(B, S, dtype=torch.int64, device=dev)
            self.tgt_lens = torch.ones(B, dtype=torch.int32, device=dev)
            self.aug = torch.zeros(B, 4, dtype=torch.int32, device=dev) if with_aug else None
        self.graph = None
        self.out = None
        self.F_cur, self.pct_cur = feats_in if feats_in is not None else (None, None)
        self.feats_out = feats_out

    def _body(self):
        ts, m = self.ts, self.ts.model
        if self.prefetch:
            nf, npct = m.arm_prefetch(self.wave, self.lens, self.dither, self.aug, out=self.feats_out, logical_len=self.logical_len)
            out = ts.step_features(self.F_cur, self.pct_cur, self.targets, self.tgt_lens, want_logp=self.want_logp, role=self.role)
            if self.feats_out is None:
                self.F_cur.copy_(nf)
                self.pct_cur.copy_(npct)
            return out
        feats, pct = ts.features(self.wave, self.lens, self.dither, self.aug, logical_len=self.logical_len)
        return ts.step_features(feats, pct, self.targets, self.tgt_lens, want_logp=self.want_logp, role=self.role)

    def capture(self, first_wave: Optional[torch.Tensor] = None, first_lens: Optional[torch.Tensor] = None, warmup: int = 2,
                first_aug: Optional[torch.Tensor] = None) -> None:
        """first_wave: the batch the first replay trains on (prefetch mode: its features are computed eagerly here; not needed
        with bound inputs + feats_in, or when ``prime()`` hands the features over).
        The eager warm-up passes and the capture pass leave the training state exactly as it was - also when the capture fails:
        they run inside ``TrainStep.preserved``, which knows what that state is."""
        ts, m = self.ts, self.ts.model
        if ts.world > 1 and not graph_dp_enabled():
            raise RuntimeError("graph capture of the data-parallel step (RCCL inside the graph) is switched off: LASR_GRAPH_DP=0")
        ts.use_device_schedule()
        if not self.bound and first_wave is not None:
            self.wave.copy_(first_wave)              # warm-up needs real audio (an all-zero wave has zero variance)
            if self.lens is not None and first_lens is not None:
                self.lens.copy_(first_lens)
            if self.aug is not None and first_aug is not None:
                self.aug.copy_(first_aug)
        # the graph's own state: the dither counter, and the first replay's features where the warm-up passes overwrite them
        own = [self.dither.step] if hasattr(self.dither, "step") else []
        if self.prefetch and self.F_cur is None:
            f, p_ = ts.features(first_wave, first_lens, None, first_aug, logical_len=self.logical_len)
            self.F_cur, self.pct_cur = f.clone(), p_.clone()
            own += [self.F_cur, self.pct_cur]
        elif self.prefetch and not self.bound and self.feats_out is None:
            own += [self.F_cur, self.pct_cur]
        with ts.preserved(own):
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream(device=m.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):            # eager warm-up on a side stream (allocator / lazy-init settle before capture)
                for _ in range(warmup):
                    self._body()
            cur.wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            # thread_local: the ingest threads (pinned allocations, H2D copies on their own stream) and RCCL's own bookkeeping may
            # call the runtime while this thread records
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):            # records the launches; nothing executes
                self.out = self._body()
            self.graph = graph

    def prime(self, feats: torch.Tensor, pct: torch.Tensor) -> None:
        """the features of the batch the next replay trains on (prefetch mode with the graph's own feature buffers)"""
        if self.F_cur is None:
            self.F_cur, self.pct_cur = feats.clone(), pct.clone()
        elif feats.data_ptr() != self.F_cur.data_ptr():
            self.F_cur.copy_(feats)
            self.pct_cur.copy_(pct)

    def step(self, wave: torch.Tensor, targets: torch.Tensor, tgt_lens: torch.Tensor, lens: Optional[torch.Tensor] = None,
             aug: Optional[torch.Tensor] = None):
        """copies the inputs into the graph's static buffers and replays; returns the static (loss, nll, logp, argmax) tensors"""
        if self.bound:
            raise RuntimeError("this graph reads its inputs in place (inputs=...): use replay()")
        self.wave.copy_(wave, non_blocking=True)
        if self.lens is not None and lens is not None:
            self.lens.copy_(lens, non_blocking=True)
        if self.aug is not None:
            if aug is not None:
                self.aug.copy_(aug, non_blocking=True)
            else:
                self.aug.zero_()
        self.targets.copy_(targets, non_blocking=True)
        self.tgt_lens.copy_(tgt_lens, non_blocking=True)
        return self.replay()

    def replay(self):
        """one training step from the captured graph (inputs as they are in the bound / static buffers right now); an
        accumulate-role graph counts a training forward and a micro-batch, but no optimiser step"""
        self.graph.replay()
        ts = self.ts
        ts.model.bump_counters(1)
        if self.role == "accumulate":
            ts.micro += 1
        else:
            ts.count_optimizer_step(advance_device=False)      # (the graph has advanced the device schedule itself)
        return self.out


def graph_dp_enabled() -> bool:
    """hipGraph capture of the data-parallel step (ncclAllReduce on the library's side stream inside the capture): on by default,
    ``LASR_GRAPH_DP=0`` keeps multi-rank steps eager"""
    return os.environ.get("LASR_GRAPH_DP", "1") != "0"


def sync_with_timeout(what: str, timeout_s: float = 180.0, hard_exit: bool = True) -> None:
    """Wait for everything enqueued on the current stream, but not for ever.  The first replay of a hipGraph that holds RCCL
    collectives is the one thing of the data-parallel step that a capture *failure* cannot catch: a replay that hangs would sit in
    ``synchronize()`` until somebody's outer limit.  On timeout the rank reports and leaves with exit code 3 (``hard_exit``; no
    re-exec, no retry - the ranks' collective sequences are unknown by then) or raises ``TimeoutError``."""
    import sys
    import time
    ev = torch.cuda.Event()
    ev.record()
    t0 = time.perf_counter()
    while not ev.query():
        if time.perf_counter() - t0 > timeout_s:
            msg = ("%s did not complete within %.0f s on rank %s - a hang inside the graph-replayed data-parallel step (RCCL collectives "
                   "captured on the library's side stream).  Re-run with LASR_GRAPH_DP=0 (eager launches) or LASR_COMM=torch "
                   "(torch.distributed's all-reduce)." % (what, timeout_s, os.environ.get("RANK", "0")))
            if not hard_exit:
                raise TimeoutError(msg)
            sys.stderr.write("lightning_asr_amd: " + msg + "\n")
            sys.stderr.flush()
            os._exit(3)
        time.sleep(0.002)
