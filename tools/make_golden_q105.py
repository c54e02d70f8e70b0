"""Generate tests/golden/model_q105.npz (mask=True) and model_q105_nomask.npz (mask=False) by running the REFERENCE's QuartNet105
(imported from the reference checkout, development container only) behind MyModel2 on formula-defined weights and inputs, and check
the helper oracle (tests/helpers/q105_oracle.py) against it while doing so - the pattern of oracle/make_golden.py.

    python tools/make_golden_q105.py <reference checkout>

Only OUTPUTS are stored (log-probs, eval log-probs, argmax, lengths, nll, losses, per-tensor gradient norms, tap checksums); weights
and inputs are regenerated from formulas on both sides.  Never imported by a test.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
from oracle import ref_cpu as R  # noqa: E402
from oracle.make_golden import check, checksum, golden_inputs  # noqa: E402
import q105_oracle as Q  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
TAPS = ["first_cnn"] + [b[0] for b in Q.BLOCKS] + ["last_cnn2"]


def run_reference(ref_root, labels, mask, x, tg, pct, tsz, n_steps=3, lr=1e-2, wd=1e-3, gain=1.0):
    sys.path.insert(0, ref_root)
    mod = importlib.import_module("models.QuartNet")
    novo = importlib.import_module("scheduler.novograd")
    n_class = len(labels) + 1
    model = mod.MyModel2(labels, 0.0, mask)
    model.encoder = mod.QuartNet105(drop_rate=0.0, mask=mask)
    shapes = Q.state_shapes(n_class)
    assert list(model.state_dict().keys()) == [k for k, _ in shapes], "state_dict key order differs from q105_oracle.state_shapes"
    for (k, shp), v in zip(shapes, model.state_dict().values()):
        assert tuple(v.shape) == tuple(shp), (k, v.shape, shp)
    assert len(shapes) == 425 and sum(p.numel() for p in model.parameters()) == 11669340
    # the quirk, read off the reference module itself
    for blk in (model.encoder.block1, model.encoder.block52):
        flags = [(bool(s.last), bool(s.mask)) for s in blk.seq]
        assert flags == [(bool(mask), True)] * 4 + [(True, bool(mask))], flags
    model.load_state_dict(Q.formula_state(n_class, gain=gain))
    out = {}
    model.eval()
    with torch.no_grad():
        out["eval_logprobs"] = model(x, pct).numpy().copy()
    model.train()
    taps, hooks = {}, []
    for name, sub in model.encoder.named_children():
        def mk(nm):
            def hook(_m, _i, o):
                taps[nm] = (o[0] if isinstance(o, tuple) else o).detach().clone()
            return hook
        hooks.append(sub.register_forward_hook(mk(name)))
    opt = novo.Novograd(model.parameters(), lr=lr, weight_decay=wd, betas=(0.8, 0.5))
    lossf = torch.nn.CTCLoss(blank=len(labels), reduction="none")
    losses = []
    for step in range(n_steps):
        opt.zero_grad()
        lp = model(x, pct)
        t_len = torch.mul(lp.size(1), pct).int()
        nll = lossf(lp.transpose(0, 1), tg, t_len, tsz)
        loss = torch.mean(nll)
        loss.backward()
        if step == 0:
            for h in hooks:
                h.remove()
            out["logprobs"] = lp.detach().numpy().copy()
            out["t_lengths"] = t_len.numpy().copy()
            out["nll"] = nll.detach().numpy().copy()
            out["argmax"] = lp.argmax(-1).to(torch.int16).numpy().copy()
            for nm, v in taps.items():
                out["tap_" + nm] = checksum(v)
            out["grad_norms"] = np.array([p.grad.norm().item() for p in model.parameters()])
            out["_grads"] = [p.grad.detach().clone() for p in model.parameters()]
        losses.append(loss.item())
        opt.step()
    out["losses"] = np.array(losses)
    out["_state_after"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return out


def run_oracle(labels, mask, x, tg, pct, tsz, n_steps=3, lr=1e-2, wd=1e-3, gain=1.0):
    n_class = len(labels) + 1
    m = Q.OracleModel(n_class, mask=mask, state=Q.formula_state(n_class, gain=gain))
    out = {}
    m.training = False
    with torch.no_grad():
        out["eval_logprobs"] = m(x, pct).numpy().copy()
    st = R.NovogradState(len(m.parameters()))
    losses = []
    for step in range(n_steps):
        if step == 0:
            m.keep_taps, m.training = True, True
            with torch.no_grad():
                lp = m(x, pct)
            t_len = R.mask_lengths(lp.size(1), pct)
            out["logprobs"] = lp.numpy().copy()
            out["nll"] = R.ctc_loss_per_sample(lp, tg, t_len, tsz, n_class - 1).numpy().copy()
            out["t_lengths"] = t_len.numpy().copy()
            for nm in TAPS:
                out["tap_" + nm] = checksum(m.taps[nm])
            m.state = Q.formula_state(n_class, gain=gain)       # undo the buffer side effects of this extra forward
            m.taps, m.keep_taps = {}, False
        loss, grads = R.train_step(m, st, x, tg, pct, tsz, lr, wd)
        if step == 0:
            out["_grads"] = grads
        losses.append(loss)
    out["losses"] = np.array(losses)
    out["_state_after"] = {k: v.detach().clone() for k, v in m.state.items()}
    return out


def margin_share(ref, labels, mask, x, pct, gain):
    """share of the valid frames whose reference top-1 / top-2 margin is below 2 x noise, noise = the helper oracle's f32 against
    its f64 evaluation (the rule tests/test_gpu_model_q105.py excuses argmax mismatches by; at most 1 % may qualify)"""
    n_class = len(labels) + 1
    lps = []
    for dt in (torch.float32, torch.float64):
        o = Q.OracleModel(n_class, mask=mask, state=Q.cast_state(Q.formula_state(n_class, gain=gain), dt))
        o.training = True
        with torch.no_grad():
            lps.append(o(x.to(dt), pct).double())
    noise = float((lps[0] - lps[1]).abs().max())
    lp = torch.from_numpy(ref["logprobs"]).double()
    top2 = lp.topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    valid = torch.arange(lp.shape[1]).view(1, -1) < torch.from_numpy(ref["t_lengths"]).long().view(-1, 1)
    share = float(((margin < 2 * noise) & valid).sum()) / float(valid.sum())
    return noise, share, float(margin[valid].min())


def oracle_grad_gap(labels, mask, x, tg, pct, tsz, gain):
    """r: the f32 helper oracle's worst per-tensor gradient distance (relative L2) from its f64 evaluation (q105_oracle.GOLDEN_GAIN)"""
    from oracle import ref_bf16 as E
    n_class = len(labels) + 1
    gs = []
    for dt in (torch.float32, torch.float64):
        o = Q.OracleModel(n_class, mask=mask, state=Q.cast_state(Q.formula_state(n_class, gain=gain), dt))
        gs.append(E.loss_and_grads(o, x.to(dt), tg, pct, tsz)[3])
    return max(((a.double() - b).norm() / (b.norm() + 1e-30)).item() for a, b in zip(*gs))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref_root = os.path.abspath(sys.argv[1])
    os.makedirs(GOLD, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    labels = [c.strip() for c in open(os.path.join(ref_root, "data", "labels.txt"))]
    assert len(labels) == 27
    x, tg, pct, tsz = golden_inputs()
    for mask, fname in ((True, "model_q105.npz"), (False, "model_q105_nomask.npz")):
        gain = Q.GOLDEN_GAIN[mask]
        print("q105 mask =", mask, "gain =", gain)
        ref = run_reference(ref_root, labels, mask, x, tg, pct, tsz, gain=gain)
        ora = run_oracle(labels, mask, x, tg, pct, tsz, gain=gain)
        for k in ("eval_logprobs", "logprobs", "nll", "t_lengths", "losses"):
            check(ref[k], ora[k], k)
        for nm in TAPS:
            check(ref["tap_" + nm], ora["tap_" + nm], "tap_" + nm)
        worst = 0.0
        for i, (g_r, g_o) in enumerate(zip(ref["_grads"], ora["_grads"])):
            rel = ((g_r - g_o).norm() / (g_r.norm() + 1e-20)).item()
            worst = max(worst, rel)
            assert rel <= 5e-3, ("grad", i, rel)
        print("  grads ok (%d tensors, worst rel-L2 %.2e)" % (len(ref["_grads"]), worst))
        worst = 0.0
        for k, v in ref["_state_after"].items():
            o = ora["_state_after"][k].double()
            rel = ((v.double() - o).norm() / (v.double().norm() + 1e-20)).item()
            worst = max(worst, rel)
            assert rel <= 2e-2, ("state_after", k, rel)
        print("  state after 3 NovoGrad steps ok (worst rel-L2 %.2e)" % worst)
        noise, share, min_margin = margin_share(ref, labels, mask, x, pct, gain)
        print("  f32-vs-f64 oracle noise %.3e; valid frames with margin < 2 noise: %.2f %% (smallest margin %.3e)"
              % (noise, 100 * share, min_margin))
        assert share <= 0.01, "more than 1 % of the frames are inside the noise: change `gain`"
        r = oracle_grad_gap(labels, mask, x, tg, pct, tsz, gain)
        print("  f32-vs-f64 oracle gradients, worst rel-L2 r = %.3e" % r)
        assert r <= 1e-2, "the f32 oracle does not reproduce the f64 one at this gain: take the next smaller one (q105_oracle.GOLDEN_GAIN)"
        save = {k: v for k, v in ref.items() if not k.startswith("_")}
        np.savez_compressed(os.path.join(GOLD, fname), **save)
        print("  wrote", fname, os.path.getsize(os.path.join(GOLD, fname)), "bytes")


if __name__ == "__main__":
    main()
