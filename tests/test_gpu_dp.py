"""GPU tier: the N>1 data-parallel step end to end.  Two ranks share the one MI355X of the test box (RCCL refuses two
ranks on one device, so the group is gloo over the same HBM tensors): each rank runs the staged backward with the
bucketed asynchronous all-reduce on its own shard of utterances, and must land on the parameters a single process gets
from the averaged per-shard gradients (DDP semantics of train.py:238 `accelerator='ddp'`: per-rank BN, mean gradient)."""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu
B, L, S, STEPS = 4, 32000, 9, 2


def _batch(rank, step):
    import bench
    return bench.synth_batch(B, L, S, 100 + 10 * step + rank, "cpu")


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lightning_asr_amd.engine import NativeModel
        from lightning_asr_amd.step import TrainStep
        dev = torch.device("cuda", 0)
        m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.float32, device=dev)
        m.init_parameters(seed=rank)                 # ranks start apart: the wrap-time broadcast must align them
        ts = TrainStep(m, 1e-2, 1e-3)
        assert ts.world == 2 and ts.overlap
        ts.broadcast_parameters()
        losses = []
        for s in range(STEPS):
            wave, tg, tl = _batch(rank, s)
            loss, *_ = ts.step(wave.to(dev), tg.to(dev), tl.to(dev))
            losses.append(float(loss.item()))
        torch.cuda.synchronize()
        q.put((rank, m.params.cpu().numpy(), losses))           # numpy: pickled by value, no fd hand-over to outlive us
    except Exception:
        import traceback
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_match_averaged_gradients(dev):
    import torch.multiprocessing as mp
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.step import TrainStep
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in res:
        assert r[1] is not None, r[2]
    res = [(r[0], torch.from_numpy(r[1]), r[2]) for r in res]
    assert torch.equal(res[0][1], res[1][1])                      # replicas stay bit-identical
    # single-process expectation: mean of the two shards' gradients from the same parameters, then NovoGrad
    m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.float32, device=dev)
    m.init_parameters(seed=0)
    ts = TrainStep(m, 1e-2, 1e-3)
    assert ts.world == 1
    for s in range(STEPS):
        g, losses = [], []
        for r in range(2):
            wave, tg, tl = _batch(r, s)
            feats, pct = ts.features(wave.to(dev))
            loss, *_ = m.loss_backward(feats, pct, tg.to(dev), tl.to(dev))
            g.append(m.grads.clone())
            losses.append(float(loss.item()))
        m.grads.copy_((g[0] + g[1]) * 0.5)
        ts.optimizer_step()
        for r in range(2):
            assert res[r][2][s] == pytest.approx(losses[r], rel=1e-5)
    got, ref = res[0][1].double(), m.params.cpu().double()
    assert torch.isfinite(got).all()
    assert ((got - ref).norm() / ref.norm()).item() < 1e-6
    assert (got - ref).abs().max().item() < 1e-5


def test_feature_prefetch_is_bit_identical(dev):
    """TrainStep.step(prefetch_wave=...) computes the next batch's log-mel in the grid of this step's CTC lattice kernel
    (lasr_ctc_loss_mel); the training trajectory must not change by a bit - also when the next call brings a different
    batch than announced."""
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.step import TrainStep
    batches = [tuple(t.to(dev) for t in _batch(0, s)) for s in range(4)]

    def run(prefetch):
        m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
        m.init_parameters(seed=3)
        ts = TrainStep(m, 1e-2, 1e-3)
        losses = []
        for s, (wave, tg, tl) in enumerate(batches):
            nxt = None
            if prefetch and s + 1 < len(batches):
                nxt = batches[s + 1][0] if s != 1 else batches[0][0]      # step 1 announces the WRONG next batch
            loss, *_ = ts.step(wave, tg, tl, prefetch_wave=nxt)
            losses.append(float(loss.item()))
        torch.cuda.synchronize()
        return m.params.clone(), losses

    p0, l0 = run(False)
    p1, l1 = run(True)
    assert l0 == l1
    assert torch.equal(p0, p1)


@pytest.mark.parametrize("variant,n_buckets", [("plain", 2), ("plain", 4), ("context_se", 2), ("context_se", 4)])
def test_native_rccl_communicator_staged_step_one_rank(dev, variant, n_buckets, monkeypatch):
    """lasr_comm_* (librccl called by the library on its own side stream, ordered by events) on a 1-rank communicator: the
    staged backward issues every bucket's ncclAllReduce from the stage boundary, the optimiser waits on the side stream.
    With one rank the all-reduce is the identity, so the trajectory must equal, bit for bit, the same staged step with the
    collectives left out - for the context variants too, whose BiLSTM parameters form the second piece of a bucket (grouped
    launch).  (Staged vs single-call backward is compared in test_gpu_model.py; in bf16 they differ in the split-K order.)"""
    from lightning_asr_amd.comm import Communicator
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.step import TrainStep
    monkeypatch.setenv("LASR_DP_BUCKETS", str(n_buckets))
    batches = [tuple(t.to(dev) for t in _batch(0, s)) for s in range(3)]

    class NoComm:                      # same staging, no collectives
        world, rank = 1, 0
        calls = 0

        def all_reduce_ranges(self, flat, ranges):
            NoComm.calls += 1

        def broadcast(self, flat, root=0):
            pass

        def wait(self):
            pass

    def run(comm):
        m = NativeModel(variant, 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
        m.init_parameters(seed=5)
        ts = TrainStep(m, 1e-2, 1e-3, comm=comm)
        ts.force_staged = True
        if not isinstance(comm, NoComm):
            ts.broadcast_parameters()
            sched = m.bucket_schedule()
            assert len(sched) == n_buckets
            covered = sorted(r for _, ranges in sched for r in ranges)
            assert covered[0][0] == 0 and covered[-1][1] == m.n_param
            assert all(a[1] == b[0] for a, b in zip(covered[:-1], covered[1:]))       # the pieces tile the flat gradient
        losses = [float(ts.step(w, tg, tl)[0].item()) for w, tg, tl in batches]
        torch.cuda.synchronize()
        return m.params.clone(), losses
    p0, l0 = run(NoComm())
    assert NoComm.calls == n_buckets * len(batches)
    comm = Communicator.single(dev)
    assert comm.world == 1 and comm.rank == 0
    p1, l1 = run(comm)
    comm.close()
    assert l0 == l1
    assert torch.equal(p0, p1)


def test_native_rccl_allreduce_orders_after_producer_stream(dev):
    """the side stream must wait for the producer's kernels and the consumer for the collective: fill -> all-reduce -> read
    on a 64 MB buffer gives the filled value on every element (a missing event edge shows up as stale zeros)"""
    from lightning_asr_amd.comm import Communicator
    comm = Communicator.single(dev)
    buf = torch.zeros(16 << 20, dtype=torch.float32, device=dev)
    for k in range(1, 4):
        buf.fill_(float(k))
        comm.all_reduce_ranges(buf, [(0, 1 << 20), (1 << 20, buf.numel())])
        comm.wait()
        assert float(buf.sum().item()) == float(k) * buf.numel()
    comm.close()


def test_device_lr_schedule_matches_host(dev):
    """lasr_lr_schedule_step (one-thread kernel, f64 state on the device) against the host class it mirrors
    (scheduler/cosine_annearing_with_warmup.py:53-89) across warm-up, cosine decay and two restarts with cycle_mult / gamma."""
    import ctypes as C
    from lightning_asr_amd import _lib
    from lightning_asr_amd.schedule import CosineAnnealingWarmupRestarts
    sc = CosineAnnealingWarmupRestarts(None, first_cycle_steps=50, cycle_mult=2, max_lr=1e-2, min_lr=1e-4, warmup_steps=10, gamma=0.5)
    nb = int(_lib.load().lasr_lr_schedule_state_bytes())
    host = C.create_string_buffer(nb)
    _lib.call("lasr_lr_schedule_init", host, nb, sc.first_cycle_steps, float(sc.cycle_mult), float(sc.base_max_lr), float(sc.min_lr),
              sc.warmup_steps, float(sc.gamma), sc.cycle, sc.step_in_cycle, sc.cur_cycle_steps, sc.last_epoch)
    state = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(dev)
    lr = torch.zeros(1, dtype=torch.float32, device=dev)
    got, exp = [], []
    for _ in range(400):
        _lib.call("lasr_lr_schedule_step", state.data_ptr(), lr.data_ptr(), torch.cuda.current_stream().cuda_stream)
        got.append(lr.clone())
        exp.append(sc.step())
    got = torch.cat(got).cpu().double()
    exp = torch.tensor(exp, dtype=torch.float64)
    assert ((got - exp).abs() / exp).max() < 2e-7          # f32 rounding of an f64 value
    assert sc.cycle >= 2                                   # the range covered at least two restarts


def test_schedule_reloaded_between_replays_restarts_the_device_twin_in_place(dev):
    """``schedule.load_state_dict`` behind the device twin's back, between two steps: the step after it notices, re-uploads the
    schedule INTO the device state a captured graph holds the address of, and advances it - replayed steps then read, step for step,
    the rate, the device state and the host position the eager steps read, and land on the same parameters."""
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.schedule import CosineAnnealingWarmupRestarts
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    batches = [tuple(t.to(dev) for t in _batch(0, s)) for s in range(5)]

    def schedule(steps=0):
        sc = CosineAnnealingWarmupRestarts(None, first_cycle_steps=50, cycle_mult=2, max_lr=1e-2, min_lr=1e-4, warmup_steps=10, gamma=0.5)
        for _ in range(steps):
            sc.step()
        return sc
    resumed = dict(schedule(17).state_dict())

    def run(graph):
        m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
        m.init_parameters(seed=9)
        ts = TrainStep(m, 1e-2, 1e-3, schedule=schedule())
        ts.use_device_schedule()
        step = ts.step
        if graph:
            g = GraphedTrainStep(ts, B, L, S, prefetch=False, want_logp=True)
            g.capture(batches[0][0])
            step = g.step
        address, seen = ts._lr_state.data_ptr(), []
        for i, (wave, tg, tl) in enumerate(batches):
            if i == 2:
                ts.schedule.load_state_dict(dict(resumed))
            step(wave, tg, tl)
            seen.append((ts.lr_dev.clone(), ts._lr_state.clone(), ts.lr, ts.schedule.last_epoch))
        torch.cuda.synchronize()
        assert ts._lr_state.data_ptr() == address             # the re-upload wrote in place
        return seen, m.params.clone()
    eager, p0 = run(False)
    replayed, p1 = run(True)
    assert [s[3] for s in eager] == [1, 2, 18, 19, 20]
    for (lr0, st0, host0, ep0), (lr1, st1, host1, ep1) in zip(eager, replayed):
        assert torch.equal(lr0.view(torch.int32), lr1.view(torch.int32)) and torch.equal(st0, st1) and host0 == host1 and ep0 == ep1
        assert abs(float(lr1) - host1) <= 2e-7 * host1        # the device's rate is the host's, to f32 rounding
    assert torch.equal(p0, p1)


@pytest.mark.parametrize("variant,prefetch", [("plain", True), ("plain", False), ("context_se", True)])
def test_graphed_step_equals_eager(dev, variant, prefetch):
    """GraphedTrainStep (the step captured into a hipGraph and replayed) against the eager TrainStep on the same batches:
    same losses, bit-identical parameters; capture itself must leave the training state untouched."""
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.schedule import CosineAnnealingWarmupRestarts
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    batches = [tuple(t.to(dev) for t in _batch(0, s)) for s in range(4)]

    def make():
        m = NativeModel(variant, 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
        m.init_parameters(seed=9)
        sc = CosineAnnealingWarmupRestarts(None, first_cycle_steps=1000, cycle_mult=2, max_lr=1e-2, min_lr=1e-4, warmup_steps=3, gamma=0.5)
        return m, TrainStep(m, 1e-2, 1e-3, schedule=sc)
    m0, ts0 = make()
    l0 = []
    for s, (w, tg, tl) in enumerate(batches):
        nxt = batches[(s + 1) % 4][0] if prefetch else None
        l0.append(float(ts0.step(w, tg, tl, prefetch_wave=nxt)[0].item()))
    m1, ts1 = make()
    p_before = m1.params.clone()
    g = GraphedTrainStep(ts1, B, L, S, prefetch=prefetch, want_logp=True)
    g.capture(batches[0][0])
    assert torch.equal(m1.params, p_before) and ts1.global_step == 0 and ts1.schedule.last_epoch == 0
    l1 = []
    for s, (w, tg, tl) in enumerate(batches):
        out = g.step(batches[(s + 1) % 4][0] if prefetch else w, tg, tl)
        l1.append(float(out[0].item()))
    torch.cuda.synchronize()
    assert l0 == l1
    assert torch.equal(m0.params, m1.params)
    assert ts1.global_step == 4 and abs(ts1.lr - ts0.lr) < 1e-12
    sd = m1.state_dict()
    assert int(sd["encoder.first_cnn.bn.num_batches_tracked"]) == 4


def _fit_worker(rank, world, port, data, out, q, stub=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      LASR_DIST_BACKEND="gloo")
    if stub:       # the library's own communicator (lasr_comm_*) over the test stand-in for librccl; gloo only carries the unique id
        os.environ["LASR_RCCL_PATH"] = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stub_rccl", "libstubrccl.so")
    try:
        from lightning_asr_amd.train import main
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        ov = ["data.train_manifest=[%s]" % os.path.join(data, "train.json"), "data.val_manifest=%s" % os.path.join(data, "dev.json"),
              "data.test_manifest=%s" % os.path.join(data, "dev.json"), "data.labels=%s" % os.path.join(root, "data", "labels.txt"),
              "train.train_batch_size=2", "train.dev_batch_size=2", "train.total_epoch=1", "train.precision=32", "train.gpus=2",
              "train.warmup_steps=2", "output_dir=%s" % os.path.join(out, "rank%d" % rank)]
        tr = main(ov)
        import torch.distributed as dist
        native = tr.fused.native
        used_comm = tr.fused.ts.comm is not None
        q.put((rank, tr.global_step, tr.history[-1]["train_loss"], str(tr.device), float(native.params.double().sum()), used_comm,
               tr.history[-1].get("val_wer"), tr.history[-1].get("val_wer_total")))
        dist.barrier()
        if used_comm:
            tr.fused.ts.comm.close()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, None, traceback.format_exc(), "", 0.0, False, None, None))


@pytest.mark.parametrize("stub", [False, True])
def test_trainer_fit_two_ranks(dev, tmp_path, stub):
    """python -m lightning_asr_amd.train with WORLD_SIZE=2 (train.py:233-252, `accelerator: ddp`): both ranks select their device
    BEFORE allocating, shard the corpus (DistributedSampler), all-reduce the flat gradient and stay in lock-step.  Two ranks
    share the test box's one GPU, so the group is gloo (LASR_DIST_BACKEND).  stub=True: the gradient exchange, the wrap-time broadcast
    and the validation metric sums go through the library's communicator (over tests/stub_rccl), as they do over RCCL on real ranks."""
    import subprocess
    import sys
    import torch.multiprocessing as mp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = str(tmp_path / "synth")
    subprocess.run([sys.executable, os.path.join(root, "tools", "make_synth_data.py"), "--out", data, "--n-train", "8", "--n-dev", "2",
                    "--seconds", "2.0"], check=True)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_fit_worker, args=(r, 2, port, data, str(tmp_path), q, stub)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(120)
    for r in res:
        assert r[1] is not None, r[2]
    assert res[0][1] == res[1][1] == 2            # 8 utterances / (2 ranks x batch 2) = 2 steps each
    assert res[0][3] == res[1][3] == "cuda:0"
    assert all(r[2] == r[2] for r in res)         # finite losses (not NaN)
    assert res[0][4] == res[1][4]                 # the replicas hold the same parameters
    assert res[0][5] == res[1][5] == stub         # lasr_comm_* carried the exchange exactly when the stub stood in for librccl
    assert res[0][6] == res[1][6] and res[0][7] == res[1][7]     # val_wer / val_wer_total agree across the ranks


def test_graphed_step_bound_inputs_ping_pong(dev):
    """two captured graphs reading resident batches in place and ping-ponging the feature buffers (what bench.py replays): no
    per-step copies, same trajectory as the eager prefetching step"""
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    batches = [tuple(t.to(dev) for t in _batch(0, s)) for s in range(2)]

    def make():
        m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
        m.init_parameters(seed=4)
        return m, TrainStep(m, 1e-2, 1e-3)
    m0, ts0 = make()
    l0 = [float(ts0.step(*batches[s % 2], prefetch_wave=batches[(s + 1) % 2][0])[0].item()) for s in range(5)]
    m1, ts1 = make()
    F0, p0 = ts1.features(batches[0][0])
    F0, p0 = F0.clone(), p0.clone()
    F1, p1 = torch.empty_like(F0), torch.empty_like(p0)
    gs = []
    for i in range(2):
        cur, nxt = batches[i], batches[1 - i]
        g = GraphedTrainStep(ts1, B, L, S, prefetch=True, want_logp=True, inputs=(nxt[0], None, cur[1], cur[2]),
                             feats_in=(F0, p0) if i == 0 else (F1, p1), feats_out=(F1, p1) if i == 0 else (F0, p0))
        g.capture()
        gs.append(g)
    f, p_ = ts1.features(batches[0][0])
    F0.copy_(f); p0.copy_(p_)
    l1 = [float(gs[s % 2].replay()[0].item()) for s in range(5)]
    torch.cuda.synchronize()
    assert l0 == l1
    assert torch.equal(m0.params, m1.params)


# ---- the library's own communicator with world == 2 -----------------------------------------------------------------------------
# Real RCCL refuses two ranks on one device and the test box has one GPU, so LASR_RCCL_PATH points lasr_comm_* at
# tests/stub_rccl/libstubrccl.so: the eight nccl* entry points comm.hip binds, implemented over hipIpc staging buffers +
# stream-ordered barriers for processes sharing a GPU.  Everything above the nccl* calls is the product path: unique-id bootstrap,
# lasr_comm_init, the side stream and its events, bucket ranges of the staged backward, broadcast, wait, 1/world in NovoGrad.
STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stub_rccl", "libstubrccl.so")


def _stub_worker(rank, world, port, q, variant, n_buckets):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LASR_RCCL_PATH=STUB,
                      LASR_DP_BUCKETS=str(n_buckets))
    dist.init_process_group("gloo", rank=rank, world_size=world)     # carries the 128-byte unique id, nothing else
    try:
        from lightning_asr_amd.comm import Communicator
        from lightning_asr_amd.engine import NativeModel
        from lightning_asr_amd.step import TrainStep
        dev = torch.device("cuda", 0)
        comm = Communicator.from_torch_distributed(dev)
        assert comm.world == 2 and comm.rank == rank
        # collectives by themselves: SUM over ranks, grouped ranges, broadcast from a non-zero root
        x = torch.arange(1000, dtype=torch.float32, device=dev) * (rank + 1)
        comm.all_reduce(x)
        y = torch.full((4096,), float(rank + 1), device=dev)
        comm.all_reduce_ranges(y, [(0, 100), (2000, 4096)])
        z = torch.full((777,), float(10 + rank), device=dev)
        comm.broadcast(z, 1)
        comm.wait()
        torch.cuda.synchronize()
        assert torch.equal(x, torch.arange(1000, dtype=torch.float32, device=dev) * 3)
        assert (y[:100] == 3).all() and (y[100:2000] == rank + 1).all() and (y[2000:] == 3).all() and (z == 11).all()
        m = NativeModel(variant, 28, mask=True, act="relu", dtype=torch.float32, device=dev)
        m.init_parameters(seed=rank)                 # ranks start apart: the wrap-time broadcast must align them
        ts = TrainStep(m, 1e-2, 1e-3, comm=comm)
        assert ts.world == 2 and ts.overlap and ts.comm is comm
        ts.broadcast_parameters()
        losses = []
        for s in range(STEPS):
            wave, tg, tl = _batch(rank, s)
            loss, *_ = ts.step(wave.to(dev), tg.to(dev), tl.to(dev))
            losses.append(float(loss.item()))
        torch.cuda.synchronize()
        q.put((rank, m.params.cpu().numpy(), losses))
        dist.barrier()
        comm.close()
    except Exception:
        import traceback
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("variant,n_buckets", [("plain", 2), ("context", 4)])
def test_library_communicator_two_ranks_over_stub_rccl(dev, variant, n_buckets):
    import torch.multiprocessing as mp
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.step import TrainStep
    assert os.path.exists(STUB), "build tests/stub_rccl/libstubrccl.so (make)"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_stub_worker, args=(r, 2, port, q, variant, n_buckets)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in res:
        assert r[1] is not None, r[2]
    res = [(r[0], torch.from_numpy(r[1]), r[2]) for r in res]
    assert torch.equal(res[0][1], res[1][1])                      # replicas stay bit-identical
    m = NativeModel(variant, 28, mask=True, act="relu", dtype=torch.float32, device=dev)
    m.init_parameters(seed=0)
    ts = TrainStep(m, 1e-2, 1e-3)
    for s in range(STEPS):
        g = []
        for r in range(2):
            wave, tg, tl = _batch(r, s)
            feats, pct = ts.features(wave.to(dev))
            loss, *_ = m.loss_backward(feats, pct, tg.to(dev), tl.to(dev))
            g.append(m.grads.clone())
            assert res[r][2][s] == pytest.approx(float(loss.item()), rel=1e-5)
        m.grads.copy_((g[0] + g[1]) * 0.5)
        ts.optimizer_step()
    got, ref = res[0][1].double(), m.params.cpu().double()
    assert torch.isfinite(got).all()
    assert ((got - ref).norm() / ref.norm()).item() < 1e-6


def _fit_unequal_worker(rank, world, port, data_dirs, out, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      LASR_DIST_BACKEND="gloo", LASR_RCCL_PATH=STUB)
    try:
        from lightning_asr_amd.train import main
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        data = data_dirs[rank]
        tr = main(["data.train_manifest=[%s]" % os.path.join(data, "train.json"), "data.val_manifest=%s" % os.path.join(data, "dev.json"),
                   "data.test_manifest=%s" % os.path.join(data, "dev.json"), "data.labels=%s" % os.path.join(root, "data", "labels.txt"),
                   "train.train_batch_size=2", "train.dev_batch_size=2", "train.total_epoch=1", "train.precision=16", "train.gpus=2",
                   "train.warmup_steps=2", "data.train_crop=false", "output_dir=%s" % os.path.join(out, "rank%d" % rank)])
        import torch.distributed as dist
        f = tr.fused
        q.put((rank, tr.global_step, f.graph_steps, f.eager_steps, f.native.params.cpu().numpy(), f.ts.comm is not None, None))
        dist.barrier()
        if f.ts.comm is not None:
            f.ts.comm.close()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, None, 0, 0, None, False, traceback.format_exc()))


def test_trainer_fit_two_ranks_capture_at_different_steps(dev, tmp_path):
    """Trainer.fit with world = 2 where the ranks see DIFFERENT batch-shape sequences: rank 0 trains on equal-length
    clips (its batch shape repeats: FusedLoop captures a hipGraph at its third occurrence and replays from then on), rank 1 on a
    ragged corpus (every batch has its own shape: it stays eager for the whole epoch).  Each rank decides on its own when to capture,
    so a capture must not issue a single collective of its own: over 12 steps per rank the bucket all-reduces of the replaying rank
    and of the eager rank pair up one to one (the stub aborts on a barrier that never fills) and the replicas end on the same bits."""
    import subprocess
    import sys
    import numpy as np
    import torch.multiprocessing as mp
    assert os.path.exists(STUB), "build tests/stub_rccl/libstubrccl.so (make)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dirs = [str(tmp_path / "equal"), str(tmp_path / "ragged")]
    for d, extra in zip(dirs, ([], ["--ragged", "--seed", "77"])):
        subprocess.run([sys.executable, os.path.join(root, "tools", "make_synth_data.py"), "--out", d, "--n-train", "48", "--n-dev", "2",
                        "--seconds", "3.0"] + extra, check=True)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_fit_unequal_worker, args=(r, 2, port, dirs, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=900) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(120)
    for r in res:
        assert r[1] is not None, r[6]
    assert res[0][1] == res[1][1] == 12           # 48 utterances / (2 ranks x batch 2)
    assert res[0][5] and res[1][5]                # lasr_comm_* (over the stub) carried the exchange
    assert res[0][2] >= 8 and res[0][3] <= 4, res[0][1:4]      # rank 0: eager until the shape came back a third time, then replays
    assert res[1][2] == 0 and res[1][3] == 12, res[1][1:4]     # rank 1: no shape ever repeats
    assert np.isfinite(res[0][4]).all() and np.array_equal(res[0][4], res[1][4])


def _stub_graph_worker(rank, world, port, q):
    """eager staged data-parallel steps vs the same steps replayed from a captured hipGraph (collectives on the library's side
    stream INSIDE the capture), two ranks over the stub"""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LASR_RCCL_PATH=STUB,
                      LASR_DP_BUCKETS="2", LASR_GRAPH_DP="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lightning_asr_amd.comm import Communicator
        from lightning_asr_amd.engine import NativeModel
        from lightning_asr_amd.step import GraphedTrainStep, TrainStep
        dev = torch.device("cuda", 0)
        comm = Communicator.from_torch_distributed(dev)
        batches = [tuple(t.to(dev) for t in _batch(rank, s)) for s in range(3)]
        out = []
        for mode in ("eager", "graph"):
            m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
            m.init_parameters(seed=5)
            ts = TrainStep(m, 1e-2, 1e-3, comm=comm)
            if mode == "eager":
                for wave, tg, tl in batches:
                    ts.step(wave, tg, tl)
            else:
                g = GraphedTrainStep(ts, B, L, S, prefetch=False, want_logp=True)
                g.capture(first_wave=batches[0][0])
                for wave, tg, tl in batches:
                    g.step(wave, tg, tl)
            torch.cuda.synchronize()
            dist.barrier()
            out.append(m.params.cpu().numpy())
        q.put((rank, out, None))
        dist.barrier()
        comm.close()
    except Exception:
        import traceback
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_data_parallel_step_replays_from_a_graph_two_ranks(dev):
    """bench.py captures the N > 1 step by default: event fork to the side stream, the bucket collectives, the join before NovoGrad
    all inside the hipGraph.  Replayed, it must land bit for bit where the eager staged step lands, on both ranks."""
    import numpy as np
    import torch.multiprocessing as mp
    assert os.path.exists(STUB), "build tests/stub_rccl/libstubrccl.so (make)"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_stub_graph_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in res:
        assert r[1] is not None, r[2]
    for r in res:
        assert np.array_equal(r[1][0], r[1][1]), "graph replay differs from eager on rank %d" % r[0]
    assert np.array_equal(res[0][1][0], res[1][1][0])            # and the replicas agree
    assert np.isfinite(res[0][1][0]).all()


def test_staged_step_with_real_rccl_replays_from_a_graph_one_rank(dev, monkeypatch):
    """the library's communicator over the REAL librccl (one rank) inside the capture: event fork to the side stream, ncclAllReduce
    (grouped ranges), join before NovoGrad - replayed, the staged step lands bit for bit where the eager staged step lands"""
    from lightning_asr_amd.comm import Communicator
    from lightning_asr_amd.engine import NativeModel
    from lightning_asr_amd.step import GraphedTrainStep, TrainStep
    monkeypatch.setenv("LASR_FORCE_OVERLAP", "1")
    monkeypatch.setenv("LASR_DP_BUCKETS", "4")
    comm = Communicator.single(dev)
    batches = [tuple(t.to(dev) for t in _batch(0, s)) for s in range(3)]
    out = []
    for mode in ("eager", "graph"):
        m = NativeModel("plain", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
        m.init_parameters(seed=6)
        ts = TrainStep(m, 1e-2, 1e-3, comm=comm)
        assert ts.force_staged and ts.comm is comm
        if mode == "eager":
            for wave, tg, tl in batches:
                ts.step(wave, tg, tl)
        else:
            g = GraphedTrainStep(ts, B, L, S, prefetch=False, want_logp=True)
            g.capture(first_wave=batches[0][0])
            for wave, tg, tl in batches:
                g.step(wave, tg, tl)
        torch.cuda.synchronize()
        out.append(m.params.clone())
    assert torch.equal(out[0], out[1])
    comm.close()


def test_bench_two_ranks_over_stub_prints_the_comm_record(dev, tmp_path):
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one rank per process), rehearsed on ONE GPU over the
    stand-in for librccl in its CU-holding mode: the N > 1 line must explain itself - which path carried the exchange, graph or
    eager, per-bucket all-reduce time on the side stream, and the wait the optimiser's stream was actually exposed to (VERDICT r3 #1c).
    The first replay of the captured step passes the watchdog."""
    import json
    import subprocess
    import sys
    assert os.path.exists(STUB), "build tests/stub_rccl/libstubrccl.so (make)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, LASR_BENCH_BACKEND="gloo", LASR_RCCL_PATH=STUB, LASR_STUB_HOLD_CUS="8", LASR_DP_BUCKETS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LASR_COMM", "LASR_GRAPH_DP", "LASR_FORCE_OVERLAP"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
                          "--batch", "8", "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                                     # ONE JSON line, relayed by rank 0's supervisor
    d = json.loads(lines[0])
    assert "torch.distributed.run" in d["launcher"]["mode"] and d["launcher"]["rung_index"] == 0    # launch.py: a worker per rank
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["hip_graph"] is True
    c = d["comm"]
    assert c["path"].startswith("lasr_comm") and c["world"] == 2 and c["staged_backward"] and c["buckets_per_step"] == 2
    assert c["timed_region_launch"].startswith("hipGraph")
    assert len(c["buckets"]) == 2
    assert c["buckets"][0]["mb"] > c["buckets"][1]["mb"] > 1.0             # 17.8 MB, then 3.4 MB (reverse layer order)
    assert abs(sum(b["mb"] for b in c["buckets"]) - 4 * 5044572 / 1e6) < 1e-3
    # the stand-in holds its CUs for latency + bytes / wire bandwidth: the bracket on the side stream cannot be shorter
    for b in c["buckets"]:
        assert b["allreduce_us"] >= 20.0 + b["mb"] * 1e3 / 85.0 - 1.0, b
    assert c["exposed_wait_us_per_step"] is not None and c["exposed_wait_us_per_step"] >= 0.0
    assert "trainer" not in d                                                 # the one-GPU sub-record stays out of the N > 1 line


def _bench_env(**kw):
    env = dict(os.environ, LASR_BENCH_BACKEND="gloo", LASR_RCCL_PATH=STUB, LASR_DP_BUCKETS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "LASR_COMM", "LASR_GRAPH_DP", "LASR_FORCE_OVERLAP", "LASR_LAUNCH_WORKER"):
        env.pop(k, None)
    env.update(kw)
    return env


def test_bench_plain_command_starts_its_own_ranks(dev):
    """`python bench.py --gpus 2` with NO outer launcher and no RANK in the environment (the form the driver uses for one GPU; the
    reference's Lightning DDP starts its per-GPU children from the plain command too, /root/reference/train.py:233-252,
    conf/conf.yaml:21,30): the parent - which never initialises the GPU - starts two fresh workers, relays rank 0's ONE JSON line and
    adds the `launcher` record.  The --full N > 1 line carries `cpu_baseline` beside `roofline` and `comm` (SURVEY 8d / VERDICT r4 1c)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--batch", "8",
                          "--full"], env=_bench_env(), capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["hip_graph"] is True
    la = d["launcher"]
    assert la["mode"].startswith("plain command") and la["rung_index"] == 0 and la["rung"] == "graph + lasr_comm"
    assert la["attempts"][0]["exit_codes"] == [0, 0]
    assert d["comm"]["path"].startswith("lasr_comm") and d["comm"]["world"] == 2
    assert d["roofline"]["frac"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1


def test_bench_plain_command_falls_down_the_ladder(dev):
    """rung 0 loses a rank (injected: the worker of rank 1 dies at once) -> the parent ends the other worker and runs rung 1 in FRESH
    processes: LASR_GRAPH_DP=0, the exchange still through lasr_comm_*; the line says which rung ran and why the first one failed."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "8",
                          "--full", "--no-cpu-baseline"], env=_bench_env(LASR_LAUNCH_FAULT="0:1"), capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    la = d["launcher"]
    assert la["rung_index"] == 1 and la["rung"] == "eager + lasr_comm" and "rank 1 exited with code 7" in la["attempts"][0]["failed"]
    assert d["config"]["hip_graph"] is False and d["config"]["launch_rung"] == 1
    assert d["comm"]["path"].startswith("lasr_comm") and d["comm"]["timed_region_launch"] == "eager"


def test_train_main_gpus_2_starts_its_own_ranks(dev, tmp_path):
    """`python -m lightning_asr_amd.train train.gpus=2` from the plain command (conf/conf.yaml:21 `gpus`, :30 `accelerator: ddp`): the
    process decides BEFORE it touches the GPU, starts two fresh ranks and returns their code; both ranks train in lock-step (rank 0's
    metrics.jsonl and checkpoint exist, the run took the 2 steps a 2-way shard of 8 utterances at batch 2 has)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = str(tmp_path / "synth")
    subprocess.run([sys.executable, os.path.join(root, "tools", "make_synth_data.py"), "--out", data, "--n-train", "8", "--n-dev", "2",
                    "--seconds", "2.0"], check=True)
    env = dict(os.environ, LASR_DIST_BACKEND="gloo", LASR_RCCL_PATH=STUB)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "LASR_COMM", "LASR_GRAPH_DP", "LASR_LAUNCH_WORKER"):
        env.pop(k, None)
    outd = str(tmp_path / "run")
    ov = ["data.train_manifest=[%s]" % os.path.join(data, "train.json"), "data.val_manifest=%s" % os.path.join(data, "dev.json"),
          "data.test_manifest=%s" % os.path.join(data, "dev.json"), "data.labels=%s" % os.path.join(root, "data", "labels.txt"),
          "train.train_batch_size=2", "train.dev_batch_size=2", "train.total_epoch=1", "train.precision=32", "train.gpus=2",
          "train.warmup_steps=2", "output_dir=%s" % outd]
    out = subprocess.run([sys.executable, "-m", "lightning_asr_amd.train"] + ov, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads(open(os.path.join(outd, "metrics.jsonl")).read().splitlines()[-1])
    assert rec["global_step"] == 2 and rec["train_loss"] == rec["train_loss"]
    assert os.path.exists(os.path.join(outd, "checkpoints", "last.ckpt"))


def test_replay_watchdog_times_out_instead_of_hanging(dev):
    """step.sync_with_timeout - what bench.py and Trainer.fit put behind the FIRST replay of a captured step that holds collectives:
    it returns as soon as the stream drains, and when the stream does not drain in time it raises (hard_exit=False) / leaves with
    exit code 3 (bench.py) with a message that names the switches to fall back with - it never blocks for ever in synchronize()."""
    import time
    from lightning_asr_amd.step import sync_with_timeout
    x = torch.zeros(1, device=dev)
    x += 1
    t0 = time.perf_counter()
    sync_with_timeout("an idle stream", timeout_s=5.0, hard_exit=False)        # drains at once
    assert time.perf_counter() - t0 < 1.0
    torch.cuda._sleep(int(3e9))                                                 # ~1.3 s of a spinning kernel on the current stream
    t0 = time.perf_counter()
    with pytest.raises(TimeoutError, match="LASR_GRAPH_DP=0"):
        sync_with_timeout("a stream that is stuck", timeout_s=0.2, hard_exit=False)
    assert 0.15 < time.perf_counter() - t0 < 1.0
    torch.cuda.synchronize()
