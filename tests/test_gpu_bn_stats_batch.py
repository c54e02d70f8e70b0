"""The single-batch form of the channel-sliced BN backward statistics kernel (LASR_BN_STATS_BATCH, csrc/norm.hip): chunks of at most 8
rows per row lane are read in one batch of loads instead of a row loop.  Every case is checked for parity against an f64 torch
reference and for bit identity between the two forms, each run in a fresh child process (the switch is read once per process)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3


def geometry(rows, C):
    """chunk geometry of the sliced pair (bn_sliced_rpc, csrc/norm.hip): rows per chunk, chunks, rows per row lane"""
    slices = C // 64
    nchunk = max(1, min(256 // slices, rows // 64))
    rpc = -(-rows // nchunk)
    return rpc, -(-rows // rpc), -(-rpc // 64)


def _rows(C, rpc, short=37):
    """rows that give chunks of `rpc` rows with a last chunk `short` rows shorter (rows is then no multiple of 64)"""
    return (256 // (C // 64)) * rpc - short


# name -> (C, rows, residual branch, act, kind, rows per lane the geometry must give)
CASES = {}
for _C in (64, 128):
    for _res in (False, True):
        _t = "C%d_%s" % (_C, "res" if _res else "plain")
        CASES["lane1_" + _t] = (_C, 4096, _res, "relu", "randn", 1)          # one row per lane: rows = 64 chunks of 64, no other choice
        CASES["lane4_" + _t] = (_C, _rows(_C, 250), _res, "relu", "randn", 4)  # the row loop's one trip; last chunk 213 rows
        CASES["lane5_" + _t] = (_C, _rows(_C, 300), _res, "relu", "randn", 5)  # the loop's second trip starts; a whole dead row in the last chunk
        CASES["lane8_" + _t] = (_C, _rows(_C, 501), _res, "relu", "randn", 8)  # the cfg2 chunk: the last size of the single batch
        CASES["lane9_" + _t] = (_C, _rows(_C, 520), _res, "relu", "randn", 9)  # one more: both switch values take the loop
CASES["lane8_C64_res_swish"] = (64, _rows(64, 501), True, "swish", "randn", 8)
CASES["lane8_C64_res_integers"] = (64, _rows(64, 501), True, "relu", "integers", 8)
CASES["lane5_C128_plain_integers"] = (128, _rows(128, 300), False, "relu", "integers", 5)
NAMES = ["dy", "dy2", "dgamma", "dbeta", "dgamma2", "dbeta2"]


def make_inputs(name, dev):
    """bf16 tensors (1, rows, C) and f32 parameters of a case, the same in every process (host generator, fixed seed).
    "randn" cases draw every element from 8 normal values rounded to bf16 (full mantissas), not from the normal distribution itself:
    a case has 7 million elements, and with continuous inputs about one of them per case has a pre-activation so close to zero that
    the f32 kernel and the f64 reference put it on different sides of the ReLU - one such flip is 4e-3 of a dbeta, 200 times the
    tolerance.  With 8 (x 8 with the residual branch) values per channel the pre-activations are a finite set that stays clear of
    zero (the test asserts min |z| > 1e-5 on the reference), so the reference is unambiguous."""
    import torch
    C, rows, has_res, act, kind, _ = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 1)
    if kind == "integers":
        # small integers, identity coefficients: every product and every sum is exact in f32, so the sums are known exactly
        mk = lambda lo, hi: torch.randint(lo, hi + 1, (1, rows, C), generator=g).float().bfloat16()   # noqa: E731
        y, y2, dout = mk(-3, 3), (mk(-3, 3) if has_res else None), mk(-2, 2)
        gam = gam2 = torch.ones(C)
        bet = bet2 = torch.zeros(C)
    else:
        mk = lambda: torch.randn(8, generator=g).bfloat16()[torch.randint(0, 8, (1, rows, C), generator=g)]   # noqa: E731
        y, y2, dout = mk(), (mk() if has_res else None), mk()
        par = lambda base: base + 0.1 * torch.randn(C, generator=g)   # noqa: E731
        gam, bet, gam2, bet2 = par(1.0), par(0.0), par(1.0), par(0.0)
    return [None if t is None else t.to(dev) for t in (y, y2, dout, gam, bet, gam2, bet2)]


def run_case(name, dev):
    """the sliced pair (sums = NULL: statistics -> apply) through the C entry points tests/test_gpu_ops.py uses"""
    import torch
    from lightning_asr_amd import ops
    C, rows, has_res, act, kind, _ = CASES[name]
    y, y2, dout, gam, bet, gam2, bet2 = make_inputs(name, dev)
    if kind == "integers":
        ident = lambda: (torch.cat([torch.ones(C), torch.zeros(C)]).to(dev), torch.cat([torch.zeros(C), torch.ones(C)]).to(dev))  # noqa: E731
        (coef, saved), (coef2, saved2) = ident(), (ident() if has_res else (None, None))      # coef = (a, b), saved = (mean, rstd)
    else:
        def fin(t, ga, be):
            f = t.reshape(rows, C).double()
            stats = torch.cat([f.sum(0), (f * f).sum(0)]).float()
            return ops.bn_finalize(stats, ga, be, torch.zeros(C, device=dev), torch.ones(C, device=dev), rows, eps=EPS)
        (coef, saved), (coef2, saved2) = fin(y, gam, bet), (fin(y2, gam2, bet2) if has_res else (None, None))
    out = ops.bn_act_bwd(dout, y, coef, saved, gam, y2, coef2, saved2, gam2 if has_res else None, act=act, fused=True)
    torch.cuda.synchronize()
    return out


def digests(out):
    import torch
    return [None if t is None else hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest() for t in out]


def child_main(path):
    import torch
    dev = torch.device("cuda:0")
    with open(path, "w") as f:
        json.dump({name: digests(run_case(name, dev)) for name in sorted(CASES)}, f)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child_main(sys.argv[1])
    sys.exit(0)


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def forms(dev, tmp_path_factory):
    """digests of every case's outputs from two fresh processes: LASR_BN_STATS_BATCH=0 (the row loop) and =1 (the single batch)"""
    d = tmp_path_factory.mktemp("bn_stats_batch")
    procs = {}
    for sw in ("0", "1"):
        env = dict(os.environ, LASR_BN_STATS_BATCH=sw)
        procs[sw] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / ("form%s.json" % sw))], env=env)
    for sw, p in procs.items():
        assert p.wait(timeout=300) == 0, "child with LASR_BN_STATS_BATCH=%s failed" % sw
    return {sw: json.load(open(d / ("form%s.json" % sw))) for sw in procs}


def reference(name, dev):
    """f64 torch autograd on the same bf16-rounded inputs: dy, dy2, dgamma, dbeta, dgamma2, dbeta2"""
    import torch
    import torch.nn.functional as F
    C, rows, has_res, act, kind, _ = CASES[name]
    y, y2, dout, gam, bet, gam2, bet2 = make_inputs(name, dev)
    leaf = lambda t: (t.double().reshape(rows, C) if t.dim() == 3 else t.double()).detach().requires_grad_(True)   # noqa: E731

    def bn(x, ga, be):
        if kind == "integers":
            return x * ga + be                      # identity coefficients: mean 0, rstd 1
        mu, var = x.mean(0), x.var(0, unbiased=False)
        return (x - mu) / torch.sqrt(var + EPS) * ga + be
    yl, gl, bl = leaf(y), leaf(gam), leaf(bet)
    z = bn(yl, gl, bl)
    if has_res:
        y2l, g2l, b2l = leaf(y2), leaf(gam2), leaf(bet2)
        z = z + bn(y2l, g2l, b2l)
    out = F.relu(z) if act == "relu" else z * torch.sigmoid(z)
    out.backward(dout.double().reshape(rows, C))
    zmin = z.detach().abs().min().item()
    if has_res:
        return (yl.grad, y2l.grad, gl.grad, bl.grad, g2l.grad, b2l.grad), zmin
    return (yl.grad, None, gl.grad, bl.grad, None, None), zmin


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def max_rel(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


@pytest.mark.parametrize("name", sorted(CASES))
def test_bn_stats_single_batch_parity_and_bit_identity(dev, forms, name):
    import torch
    C, rows, has_res, act, kind, lanes = CASES[name]
    rpc, nchunk, rpl = geometry(rows, C)
    assert rpl == lanes and rows >= 4096, (rpc, nchunk, rpl)
    if lanes > 1:
        assert rows % 64 != 0 and rows - (nchunk - 1) * rpc < rpc          # a short last chunk
    got = run_case(name, dev)
    # (b) bit identity: the row loop and the single batch in fresh processes, and this process (the default), all the same bytes
    mine = digests(got)
    assert forms["0"][name] == forms["1"][name], [n for n, a, b in zip(NAMES, forms["0"][name], forms["1"][name]) if a != b]
    assert mine == forms["1"][name]
    # (a) parity against f64
    ref, zmin = reference(name, dev)
    if kind == "integers":
        # identity coefficients are not a BatchNorm of these inputs, so only the statistics pass is comparable: its sums, exact
        for n, t, r in zip(NAMES, got, ref):
            if n.startswith("dg") or n.startswith("db"):
                assert (t is None) == (r is None)
                if t is not None:
                    assert r.abs().max() < 2 ** 24 and torch.equal(t.double(), r), (n, (t.double() - r).abs().max().item())
        return
    # tolerances of this op in tests/test_gpu_ops.py (test_bn_act_fwd_bwd_bf16, lines 905-909): data gradients 3e-4 relative L2
    # against the bf16-rounded reference, parameter gradients 2e-5 of the largest
    assert act != "relu" or zmin > 1e-5, ("the inputs must keep every pre-activation clear of the ReLU's corner", zmin)
    for n, t, r in zip(NAMES, got, ref):
        assert (t is None) == (r is None), n
        if t is None:
            continue
        if n.startswith("dy"):
            e = rel_l2(t.reshape(rows, C).float(), r.float().bfloat16().float())
            print(name, n, "rel_l2 %.3e" % e)
            assert e < 3e-4, (n, e)
        else:
            e = max_rel(t, r)
            print(name, n, "max_rel %.3e" % e)
            assert e < 2e-5, (n, e)
