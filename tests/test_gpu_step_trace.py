"""The call trace of one training step: the ordered names of the C-ABI entry points a settled ``TrainStep.step`` fetches from
liblasr, for every way the step can be put together (K = 1 / K = 2 accumulate and boundary; unstaged, staged over torch.distributed,
staged over the library communicator; EMA + clip-by-norm + the non-finite guard off and on; ``TrainStep(...)`` and
``TrainStep.from_optimizer(...)``), against the lists in tests/golden/step_trace.json.  The Python that drives the step may be
rearranged freely; the launches it issues, and their order, may not.

The golden file holds names only.  It is what ``python tests/test_gpu_step_trace.py OUT.json`` writes on the commit whose trace is the
standard (recorded on the commit before the optimiser-state record / exchange / step-body refactor).

Beside the trace, per case: ``from_optimizer`` allocates no parameter-sized buffer (the moments, the average and the records ARE
the optimiser's), and K = 1 never allocates the micro-batch gradient buffer."""
import contextlib
import itertools
import json
import os
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)           # (run as a script, to print the golden file)
from oracle import ref_cpu as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_trace.json")
LABELS = [c.strip() for c in open(os.path.join(ROOT, "data", "labels.txt")).readlines()]
B, L, S = 2, 16000, 5              # the batch of test_gpu_grad_accum.py: two one-second utterances, T_in = 101

FEATURES = {"off": {}, "on": dict(ema_decay=0.9, gradient_clip_val=1.0, gradient_clip_algorithm="norm", skip_nonfinite=True)}
# owner x K x exchange x features.  exchange: "flat" - one call for the whole backward, no collective at world 1;
# "dist" - the staged backward with torch.distributed's asynchronous all-reduce per bucket (a one-rank gloo group);
# "comm" - the staged backward with the library's communicator (a one-rank RCCL communicator)
CASES = ["%s-K%d-%s-%s" % c for c in itertools.product(("direct", "optimizer"), (1, 2), ("flat", "dist", "comm"), ("off", "on"))]


class _Recorder:
    """stands in for the loaded library: notes the name of every entry point fetched from it, hands the real one over"""

    def __init__(self, lib):
        self.lib, self.names = lib, None

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if self.names is not None:
            self.names.append(name)
        return fn


def _schedule():
    from lightning_asr_amd.schedule import CosineAnnealingWarmupRestarts
    return CosineAnnealingWarmupRestarts(None, first_cycle_steps=100, cycle_mult=2, max_lr=1e-2, min_lr=1e-4, warmup_steps=3, gamma=0.5)


@contextlib.contextmanager
def _exchange(kind, dev):
    """(communicator | None) for the case; "dist" holds a one-rank gloo group open for the block"""
    import torch.distributed as dist
    from lightning_asr_amd.comm import Communicator
    if kind == "comm":
        comm = Communicator.single(dev)
        try:
            yield comm
        finally:
            comm.close()
    elif kind == "dist":
        with tempfile.TemporaryDirectory() as d:
            dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "store"), rank=0, world_size=1)
            try:
                yield None
            finally:
                dist.destroy_process_group()
    else:
        yield None


def _build(dev, owner, K, comm, feat):
    """the TrainStep of a case over the smallest model the accumulation tests build (plain, bf16).  "direct": it owns its state and
    steps the host schedule; "optimizer": over a Novograd's state with the schedule on the device, as Trainer.fit sets it up"""
    from lightning_asr_amd.step import TrainStep
    if owner == "direct":
        from lightning_asr_amd.engine import NativeModel
        m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
        m.init_parameters(seed=5)
        return TrainStep(m, 1e-2, 1e-3, schedule=_schedule(), comm=comm, accumulate=K, **feat)
    from lightning_asr_amd.scheduler.novograd import Novograd
    from lightning_asr_amd.train import LightingModule
    lm = LightingModule(learning_rate=1e-2, weight_decay=1e-3, labels=LABELS, total_epoch=1, drop_rate=0.0, mask=True, use_cer=True,
                        dtype="bf16", device=str(dev))
    m = lm.encoder.native
    opt = Novograd(lm.parameters(), lr=1e-2, weight_decay=1e-3, betas=(0.8, 0.5), **feat)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    ts = TrainStep.from_optimizer(m, opt, _schedule(), comm=comm, accumulate=K)
    peak, after = torch.cuda.max_memory_allocated(dev) - before, torch.cuda.memory_allocated(dev) - before
    # a zeros_like(params) that is allocated and dropped, or kept, is 4 bytes x n_param; what the step may own beside the
    # optimiser's state is a few small records - a quarter of ONE such buffer is far above those and far below any copy
    ts.construction_bytes = (peak, after, m.params.numel())        # (peak growth, kept growth, the bound): asserted by the test
    assert ts.exp_avg is opt.exp_avg and ts.exp_avg_sq is opt.exp_avg_sq and ts.lr_dev is opt.lr_dev
    assert ts.ema is opt.ema and ts.ema_state is opt.ema_state and ts.clip_state is opt.clip_state
    ts.use_device_schedule()
    ts._keep = (lm, opt)
    return ts


def _trace(dev, case, install, check_memory=True):
    """{role: [entry-point names]} of the settled step(s) of a case.  install(recorder) puts the recorder where ``_lib.load()``
    finds it."""
    from lightning_asr_amd import _lib
    owner, K, kind, feat = case.split("-")
    K = int(K[1:])
    batches = []
    for s in range(2 * K):
        wave, tg, tl = R.synth_batch(B, L, S, 27, seed=300 + s)
        batches.append((wave.to(dev), tg.to(dev), tl.to(dev)))
    rec = _Recorder(_lib.load())
    install(rec)
    out = {}
    with _exchange(kind, dev) as comm:
        ts = _build(dev, owner, K, comm, FEATURES[feat])
        if kind != "flat":
            ts.force_staged = True
        if owner == "optimizer" and check_memory:
            peak, kept, bound = ts.construction_bytes
            assert peak < bound and kept < bound, (peak, kept, bound)
        assert ts.world == 1 and ts.comm is comm
        for b in batches[:K]:              # one warm-up optimiser step: workspaces and lazy state settle
            ts.step(*b)
        for i, b in enumerate(batches[K:]):
            rec.names = []
            ts.step(*b)
            out["boundary" if i == K - 1 else "accumulate"], rec.names = rec.names, None
        torch.cuda.synchronize()
        assert ts.global_step == 2 and ts.micro == 0
        if K == 1:
            assert ts.model._grads_micro is None       # K = 1: no second gradient buffer, ever
        if feat == "on":
            assert ts.ema_num_updates == 2 and ts.skipped_steps == 0
    return out


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_step_issues_the_recorded_calls_in_the_recorded_order(dev, case, golden, monkeypatch):
    from lightning_asr_amd import _lib
    for k in ("LASR_FORCE_OVERLAP", "LASR_COMM", "LASR_ROCTX", "LASR_RCCL_PATH"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LASR_DP_BUCKETS", "2")
    got = _trace(dev, case, lambda rec: monkeypatch.setattr(_lib, "_lib", rec))
    assert sorted(got) == sorted(golden[case])
    for role, names in got.items():
        assert names == golden[case][role], (case, role)


def test_the_cases_differ_where_the_step_differs(golden):
    """(no GPU needed) the golden lists are not vacuous: the staged step, the accumulate launch, the communicator and the EMA / clip entry each
    leave their mark"""
    assert sorted(golden) == sorted(CASES)
    g = golden
    assert "lasr_model_loss_backward" in g["direct-K1-flat-off"]["boundary"]
    assert "lasr_model_backward_continue" in g["direct-K1-dist-off"]["boundary"]
    assert "lasr_comm_allreduce_ranges" in g["direct-K1-comm-off"]["boundary"] and "lasr_comm_wait" in g["direct-K1-comm-off"]["boundary"]
    assert "lasr_comm_allreduce_ranges" not in g["direct-K2-comm-off"]["accumulate"]
    assert "lasr_grad_accumulate" in g["direct-K2-flat-off"]["accumulate"] and "lasr_grad_accumulate_ranges" in g["direct-K2-dist-off"]["accumulate"]
    assert not any(n.startswith("lasr_novograd_step") for n in g["direct-K2-flat-on"]["accumulate"])
    assert "lasr_novograd_step_keep" in g["direct-K1-flat-off"]["boundary"] and "lasr_novograd_step_clip" in g["direct-K1-flat-on"]["boundary"]
    assert "lasr_lr_schedule_step" in g["optimizer-K1-flat-off"]["boundary"] and "lasr_lr_schedule_step" not in g["direct-K1-flat-off"]["boundary"]


if __name__ == "__main__":          # python tests/test_gpu_step_trace.py OUT.json: the golden file's content, from the checked-out tree
    from lightning_asr_amd import _lib
    os.environ["LASR_DP_BUCKETS"] = "2"
    real = _lib.load()
    traces = {}
    for c in CASES:
        try:
            traces[c] = _trace(torch.device("cuda:0"), c, lambda rec: setattr(_lib, "_lib", rec), check_memory=False)
        finally:
            _lib._lib = real
    with open(sys.argv[1], "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(c), json.dumps(traces[c], sort_keys=True)) for c in sorted(traces)) + "\n}\n")
