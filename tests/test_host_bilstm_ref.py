"""CPU tier of the BiLSTM operator tests: the reference of tests/helpers/bilstm_ref.py (what tests/test_gpu_lstm.py holds the HIP
kernels to) against torch.nn.LSTM in f64, and the reference's own f32-vs-f64 distance on the GPU tests' case tables - the floor
any f32 implementation of the operator sits at (profiles/lstm_op_parity.json, "cpu_f32_floor")."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bilstm_ref as L  # noqa: E402

PROFILE = os.path.join(ROOT, "profiles", "lstm_op_parity.json")
# the ceilings of the GPU tests (tests/test_gpu_units.py TOL["f32"]: act 5e-6, grad_param 2e-5)
CEIL = {"out": 5e-6, "gates": 5e-6, "c": 5e-6, "h": 5e-6, "dg": 2e-5, "dwhh": 2e-5}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_bilstm_ref_matches_torch_lstm_f64():
    """pack_padded_sequence -> nn.LSTM(256, 40, bidirectional, batch_first) -> pad_packed_sequence in f64, ragged lengths with
    1, 8, 9 and T: output, d/dx, d/dW_ih, d/dW_hh and both bias gradients to 1e-12 relative.  Pins the reference's gate order,
    the bias sum, the reverse direction's start at len - 1 and the zero output past len."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    torch.manual_seed(3)
    B, T = 6, 12
    lens = [12, 1, 8, 9, 5, 12]
    lstm = torch.nn.LSTM(256, 40, bidirectional=True, batch_first=True).double()
    x = torch.randn(B, T, 256, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(B, T, 80, dtype=torch.float64)
    y, _ = pad_packed_sequence(lstm(pack_padded_sequence(x, torch.tensor(lens), batch_first=True, enforce_sorted=False))[0],
                               batch_first=True, total_length=T)
    (y * dout).sum().backward()
    p = dict(lstm.named_parameters())
    wih = torch.stack([p["weight_ih_l0"], p["weight_ih_l0_reverse"]]).detach()
    whh = torch.stack([p["weight_hh_l0"], p["weight_hh_l0_reverse"]]).detach()
    bih = torch.stack([p["bias_ih_l0"], p["bias_ih_l0_reverse"]]).detach()
    bhh = torch.stack([p["bias_hh_l0"], p["bias_hh_l0_reverse"]]).detach()
    xd = x.detach()
    dout_nan = dout.clone()
    for b, n in enumerate(lens):
        dout_nan[b, n:] = float("nan")                        # rows past len must not be read
    r = L.bilstm_ref(xd @ wih[0].t(), xd @ wih[1].t(), whh, bih, bhh, lens, dout_nan)
    assert _rel(r["out"], y.detach()) < 1e-12
    for b, n in enumerate(lens):
        assert bool((r["out"][b, n:] == 0).all()) and bool((r["dg"][:, b, n:] == 0).all())
    dx = r["dg"][0] @ wih[0] + r["dg"][1] @ wih[1]
    assert _rel(dx, x.grad) < 1e-12
    sfx = ["", "_reverse"]
    for d in range(2):
        assert _rel(r["dwhh"][d], p["weight_hh_l0" + sfx[d]].grad) < 1e-12
        assert _rel(r["dg"][d].reshape(-1, 160).t() @ xd.reshape(-1, 256), p["weight_ih_l0" + sfx[d]].grad) < 1e-12
        assert _rel(r["dbias"][d], p["bias_ih_l0" + sfx[d]].grad) < 1e-12
        assert _rel(r["dbias"][d], p["bias_hh_l0" + sfx[d]].grad) < 1e-12
        assert _rel(r["dg"][d].sum((0, 1)), r["dbias"][d]) < 1e-12      # db = colsum(dg), as include/lasr.h states it


def test_bilstm_ref_length_zero_and_clamp():
    """length 0 is not packable: the reference must give all zeros and zero gradient for it, leave the other utterances
    unchanged, and clamp lens > T to T"""
    inp = L.make_inputs(3, 5, seed=9)
    a = (inp["gx_f"], inp["gx_r"], inp["whh"], inp["bias_ih"], inp["bias_hh"])
    r0 = L.bilstm_ref(*a, [0, 3, 9], inp["dout"])
    r1 = L.bilstm_ref(*a, [2, 3, 5], inp["dout"])
    assert bool((r0["out"][0] == 0).all()) and bool((r0["dg"][:, 0] == 0).all()) and bool((r0["gates"][0] == 0).all())
    assert torch.equal(r0["out"][1:], r1["out"][1:]) and torch.equal(r0["dg"][:, 1:], r1["dg"][:, 1:])
    rz = L.bilstm_ref(*a, [0, 0, 0], inp["dout"])
    for k in ("out", "dg", "dwhh", "dbias"):
        assert bool((rz[k] == 0).all()), k


def test_comparators_propagate_nan():
    """a NaN in either direction, in any utterance, must come out of the comparators as NaN (the GPU tests prefill with NaN so
    that an unwritten element shows; Python's max() would drop it)"""
    _, lens = L.case("len9")
    ref = L.case_ref("len9")
    assert L.worst_of([1.0, float("nan"), 2.0]) != L.worst_of([1.0, float("nan"), 2.0]) and L.worst_of([1.0, 3.0, 2.0]) == 3.0
    for q, idx in (("out", (0, 8, 79)), ("dg", (1, 0, 8, 159)), ("h", (0, 3, 1, 39))):
        got = {k: v.clone() for k, v in ref.items()}
        assert L.worst_per_utterance(got, ref, lens, q) == 0.0
        got[q][idx] = float("nan")
        w = L.worst_per_utterance(got, ref, lens, q)
        assert w != w, q


def test_bilstm_ref_f32_floor_on_the_gpu_case_tables():
    """the reference in f32 against itself in f64 on every case of the GPU tests, worst per (utterance, direction) relative L2 per
    quantity: the distance that f32 storage and arithmetic alone put between two correct implementations.  The figures are
    orientation, not a gate on any kernel.  Two assertions are this test's own additions, kept on purpose: the floor sits below
    half of the GPU tests' ceilings (CEIL above repeats them: a ceiling must not ask for more than the format gives), and
    profiles/lstm_op_parity.json holds a floor for exactly these cases and quantities - so the test needs that file.  An
    ordinary run only reads it; LASR_LSTM_RECORD_FLOOR=1 is the one way the committed record is rewritten, from that run."""
    floor = {}
    for name in L.FLOOR_CASES:
        _, lens = L.case(name)
        r64, r32 = L.case_ref(name, torch.float64), L.case_ref(name, torch.float32)
        cur = {q: L.worst_per_utterance(r32, r64, lens, q) for q in ("out", "gates", "c", "h", "dg")}
        if max(lens) > 1:
            cur["dwhh"] = L.worst_of(L.rel_l2(r32["dwhh"][d], r64["dwhh"][d]) for d in range(2))
        else:
            assert bool((r64["dwhh"] == 0).all()) and bool((r32["dwhh"] == 0).all())
        group = "per_length" if name.startswith("len") else name
        for q, v in cur.items():
            floor.setdefault(group, {})[q] = L.worst_of([floor.get(group, {}).get(q, 0.0), v])
    print("cpu_f32_floor", json.dumps(floor))
    for group, qs in floor.items():
        for q, v in qs.items():
            assert v < 0.5 * CEIL[q], (group, q, v)
    rec = json.load(open(PROFILE))
    if os.environ.get("LASR_LSTM_RECORD_FLOOR"):
        rec["cpu_f32_floor"] = floor
        with open(PROFILE, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
    assert {g: sorted(v) for g, v in rec["cpu_f32_floor"].items()} == {g: sorted(v) for g, v in floor.items()}
