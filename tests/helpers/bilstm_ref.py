"""The BiLSTM context operator of include/lasr.h (lasr_bilstm_fwd / lasr_bilstm_bwd) as a plain per-utterance loop in any
precision, and a launcher that calls the two HIP entry points with every output prefilled.

Operator (models/QuartNetContext.py:171-173,186-199: pack_padded_sequence -> nn.LSTM(256, 40, bidirectional) ->
pad_packed_sequence): gx_f / gx_r (B, T, 160) = x W_ih^T per direction WITHOUT the biases, gate order i, f, g, o, hidden 40;
the reverse direction starts at min(lens[b], T) - 1; outputs are zero for t >= len.  The reference is checked against
torch.nn.LSTM in tests/test_host_bilstm_ref.py."""
import ctypes as C

import torch

H, G = 40, 160
SAVED = G + 2 * H          # saved [B][T][2][gates(i,f,g,o) | c | h]
OUT_SENTINEL = -768.0      # exactly representable in bf16; no LSTM output (|h| < 1) can equal it


def bilstm_ref(gx_f, gx_r, whh, bias_ih, bias_hh, lens, dout=None, dtype=torch.float64):
    """gx_f, gx_r (B, T, 160); whh (2, 160, 40); bias_ih, bias_hh (2, 160); lens (B,) integers >= 0 (clamped to T);
    dout (B, T, 80) or None.  Everything is computed in `dtype` on the CPU.

    Returns a dict: out (B, T, 80) [forward | reverse], gates (B, T, 2, 160) post-activation, c and h (B, T, 2, 40) - all zero
    for t >= len - and, with dout, by autograd of sum_{t < len} out * dout: dg (2, B, T, 160) = d/d gx per direction (zero for
    t >= len), dwhh (2, 160, 40), dbias (2, 160) (the gradient of b_ih and of b_hh alike).  Rows of dout at t >= len are never
    read, so whatever they hold (NaN included) influences nothing."""
    B, T, _ = gx_f.shape
    want_grad = dout is not None
    gx = [gx_f.detach().to(dtype).cpu().clone().requires_grad_(want_grad), gx_r.detach().to(dtype).cpu().clone().requires_grad_(want_grad)]
    w = whh.detach().to(dtype).cpu().clone().requires_grad_(want_grad)
    bi = bias_ih.detach().to(dtype).cpu().clone().requires_grad_(want_grad)
    bh = bias_hh.detach().to(dtype).cpu().clone().requires_grad_(want_grad)
    out = torch.zeros(B, T, 2 * H, dtype=dtype)
    gates = torch.zeros(B, T, 2, G, dtype=dtype)
    cs = torch.zeros(B, T, 2, H, dtype=dtype)
    hs = torch.zeros(B, T, 2, H, dtype=dtype)
    loss = torch.zeros((), dtype=dtype)
    for b in range(B):
        n = min(int(lens[b]), T)
        for d in range(2):
            h = torch.zeros(H, dtype=dtype)
            c = torch.zeros(H, dtype=dtype)
            hcol = [None] * n
            for s in range(n):
                t = n - 1 - s if d else s
                pre = gx[d][b, t] + bi[d] + bh[d] + w[d] @ h
                i, f, o = torch.sigmoid(pre[:H]), torch.sigmoid(pre[H:2 * H]), torch.sigmoid(pre[3 * H:])
                g = torch.tanh(pre[2 * H:3 * H])
                c = f * c + i * g
                h = o * torch.tanh(c)
                hcol[t] = h
                with torch.no_grad():
                    gates[b, t, d] = torch.cat([i, f, g, o])
                    cs[b, t, d] = c
                    hs[b, t, d] = h
            if n:
                hseq = torch.stack(hcol)
                with torch.no_grad():
                    out[b, :n, d * H:(d + 1) * H] = hseq
                if want_grad:
                    loss = loss + (hseq * dout[b, :n, d * H:(d + 1) * H].detach().to(dtype).cpu()).sum()
    res = {"out": out, "gates": gates, "c": cs, "h": hs}
    if want_grad:
        if loss.requires_grad and loss.grad_fn is not None:
            loss.backward()
        z = torch.zeros
        res["dg"] = torch.stack([gx[0].grad if gx[0].grad is not None else z(B, T, G, dtype=dtype),
                                 gx[1].grad if gx[1].grad is not None else z(B, T, G, dtype=dtype)])
        res["dwhh"] = w.grad if w.grad is not None else z(2, G, H, dtype=dtype)
        res["dbias"] = bi.grad if bi.grad is not None else z(2, G, dtype=dtype)
    return res


def make_inputs(B, T, seed, gx_scale=1.0):
    """the seeded inputs of the operator tests: gx ~ N(0, 1) (times gx_scale), W_hh and the biases uniform in +-1/sqrt(40),
    dout ~ N(0, 1); all f32 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / H ** 0.5
    return {"gx_f": gx_scale * torch.randn(B, T, G, generator=g), "gx_r": gx_scale * torch.randn(B, T, G, generator=g),
            "whh": (2 * torch.rand(2, G, H, generator=g) - 1) * k, "bias_ih": (2 * torch.rand(2, G, generator=g) - 1) * k,
            "bias_hh": (2 * torch.rand(2, G, generator=g) - 1) * k, "dout": torch.randn(B, T, 2 * H, generator=g)}


def _code(dtype):
    from lightning_asr_amd import _lib
    return {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}[dtype]


def bilstm_gpu_fwd(dev, gx_f, gx_r, whh, bias_ih, bias_hh, lens, ld=2 * H, col0=0, dtype=torch.float32):
    """lasr_bilstm_fwd.  Returns (out (B, T, ld) of `dtype`, prefilled with OUT_SENTINEL; saved (B, T, 2, 240) f32, prefilled
    with NaN).  Every device operand is held in a variable until after the synchronize (a temporary's block would be reused)."""
    from lightning_asr_amd import _lib
    from lightning_asr_amd.ops import _p, _stream
    B, T, _ = gx_f.shape
    gf, gr = gx_f.float().contiguous().to(dev), gx_r.float().contiguous().to(dev)
    w = whh.float().contiguous().to(dev)
    bi, bh = bias_ih.float().contiguous().to(dev), bias_hh.float().contiguous().to(dev)
    lens_d = torch.as_tensor(lens, dtype=torch.int32).to(dev)
    out = torch.full((B, T, ld), OUT_SENTINEL, dtype=dtype, device=dev)
    assert _lib.load().lasr_bilstm_saved_bytes(B, T) == B * T * 2 * SAVED * 4
    saved = torch.full((B, T, 2, SAVED), float("nan"), dtype=torch.float32, device=dev)
    wf, wr, bif, bir, bhf, bhr = w[0], w[1], bi[0], bi[1], bh[0], bh[1]
    _lib.call("lasr_bilstm_fwd", _p(gf), _p(gr), _p(wf), _p(wr), _p(bif), _p(bhf), _p(bir), _p(bhr), _p(lens_d), B, T, _p(out),
              _code(dtype), ld, col0, _p(saved), _stream())
    torch.cuda.synchronize()
    return out, saved


def bilstm_gpu_bwd(dev, dout_full, whh, lens, saved, ld, col0):
    """lasr_bilstm_bwd on a d(out) tensor (B, T, ld) of f32 or bf16 whose columns [col0, col0 + 80) hold the gradient.  Returns
    dg_f, dg_r (B, T, 160) (prefilled with NaN), dwhh_f, dwhh_r (160, 40) (prefilled with NaN).  The workspace is exactly
    lasr_bilstm_bwd_workspace_bytes(B)."""
    from lightning_asr_amd import _lib
    from lightning_asr_amd.ops import _p, _stream
    B, T, ldd = dout_full.shape
    assert ldd == ld and dout_full.dtype in (torch.float32, torch.bfloat16)
    do = dout_full.contiguous().to(dev)
    w = whh.float().contiguous().to(dev)
    lens_d = torch.as_tensor(lens, dtype=torch.int32).to(dev)
    nan = float("nan")
    dg_f = torch.full((B, T, G), nan, dtype=torch.float32, device=dev)
    dg_r = torch.full((B, T, G), nan, dtype=torch.float32, device=dev)
    dw_f = torch.full((G, H), nan, dtype=torch.float32, device=dev)
    dw_r = torch.full((G, H), nan, dtype=torch.float32, device=dev)
    wsb = int(_lib.load().lasr_bilstm_bwd_workspace_bytes(B))
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev)       # (all-ones bytes: NaN as f32)
    wf, wr = w[0], w[1]
    sv = saved.contiguous()
    _lib.call("lasr_bilstm_bwd", _p(do), _code(do.dtype), ld, col0, _p(wf), _p(wr), _p(lens_d), B, T, _p(sv), _p(dg_f), _p(dg_r),
              _p(dw_f), _p(dw_r), _p(ws), C.c_size_t(wsb), _stream())
    torch.cuda.synchronize()
    return dg_f, dg_r, dw_f, dw_r


def bilstm_gpu(dev, gx_f, gx_r, whh, bias_ih, bias_hh, lens, dout, ld=2 * H, col0=0, dtype=torch.float32, dout_pad=0.0):
    """forward then backward through the C ABI.  dout (B, T, 80) is placed into columns [col0, col0 + 80) of a (B, T, ld) tensor
    of `dtype` whose other columns hold dout_pad.  Returns a dict of CPU tensors: out_full (B, T, ld), out (B, T, 80) (the column
    window), saved (B, T, 2, 240), dg (2, B, T, 160), dwhh (2, 160, 40)."""
    B, T, _ = gx_f.shape
    out, saved = bilstm_gpu_fwd(dev, gx_f, gx_r, whh, bias_ih, bias_hh, lens, ld, col0, dtype)
    dfull = torch.full((B, T, ld), dout_pad, dtype=dtype)
    dfull[:, :, col0:col0 + 2 * H] = dout.to(dtype)
    dg_f, dg_r, dw_f, dw_r = bilstm_gpu_bwd(dev, dfull, whh, lens, saved, ld, col0)
    out_c = out.cpu()
    return {"out_full": out_c, "out": out_c[:, :, col0:col0 + 2 * H], "saved": saved.cpu(),
            "dg": torch.stack([dg_f.cpu(), dg_r.cpu()]), "dwhh": torch.stack([dw_f.cpu(), dw_r.cpu()])}


# ---- the case tables shared by tests/test_host_bilstm_ref.py (the f32-vs-f64 floor of the reference) and tests/test_gpu_lstm.py ----

# every length class of the kernels: 0 (nothing runs, clamped priming loads), 1 (no previous state anywhere), below / at / above
# one round of the kPre = 8 register ring, len % 8 in {0, 1, 7}, and len - 1 around the 16-way dW_hh split (15, 16, 17, 31, 32, 33)
EDGE_LENS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 18, 23, 24, 25, 31, 32, 33, 34]
EDGE_T = 36


def case(name):
    """(inputs dict of make_inputs, lens list) of a named case"""
    if name == "edges":
        return make_inputs(len(EDGE_LENS), EDGE_T, seed=101), list(EDGE_LENS)
    if name.startswith("len"):                    # one utterance of that length, two padded frames behind it
        n = int(name[3:])
        return make_inputs(1, n + 2, seed=200 + n), [n]
    if name == "long_801_501":
        return make_inputs(2, 801, seed=301), [801, 501]
    if name == "long_2001":
        return make_inputs(1, 2001, seed=302), [2001]
    if name == "saturated":
        inp = make_inputs(2, 40, seed=401, gx_scale=12.0)
        # exp() overflows to inf inside sigmoid_fast / tanh_fast: one entry per gate kind and sign, both directions, both utterances
        inp["gx_f"][0, 5, 3] = 1e4
        inp["gx_f"][0, 7, H + 3] = -1e4
        inp["gx_f"][1, 20, 2 * H + 9] = -1e4
        inp["gx_f"][1, 21, 2 * H + 11] = 1e4
        inp["gx_r"][1, 10, 2 * H + 5] = 1e4
        inp["gx_r"][1, 12, 3 * H + 7] = -1e4
        inp["gx_r"][0, 30, 17] = -1e4
        inp["gx_r"][0, 2, H + 21] = 1e4
        return inp, [40, 33]
    raise KeyError(name)


FLOOR_CASES = ["edges"] + ["len%d" % n for n in EDGE_LENS] + ["long_801_501", "long_2001", "saturated"]

_REF = {}


def case_ref(name, dtype=torch.float64):
    """bilstm_ref of a named case, computed once per process and shared (callers must not modify it)"""
    key = (name, dtype)
    if key not in _REF:
        inp, lens = case(name)
        _REF[key] = bilstm_ref(inp["gx_f"], inp["gx_r"], inp["whh"], inp["bias_ih"], inp["bias_hh"], lens, inp["dout"], dtype=dtype)
    return _REF[key]


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def worst_of(values):
    """the largest of the values, NaN as soon as one of them is NaN (Python's max() drops a NaN that is not its first argument, so
    a NaN from a kernel or from a prefill would otherwise read as 0)"""
    worst = 0.0
    for v in values:
        if v != v:
            return float("nan")
        worst = max(worst, v)
    return worst


def worst_per_utterance(got, ref, lens, what):
    """worst relative L2 over (utterance, direction) of one quantity, taken over t < len only - a short utterance is not averaged
    away by a long one.  got / ref: dicts with out (B, T, 80), gates / c / h (B, T, 2, .), dg (2, B, T, 160).  len 0: nothing to
    compare.  A NaN anywhere in t < len makes the result NaN (worst_of)."""
    errs = []
    for b, n in enumerate(lens):
        n = min(int(n), ref["out"].shape[1])
        if n == 0:
            continue
        for d in range(2):
            if what == "out":
                e = rel_l2(got["out"][b, :n, d * H:(d + 1) * H], ref["out"][b, :n, d * H:(d + 1) * H])
            elif what == "dg":
                e = rel_l2(got["dg"][d, b, :n], ref["dg"][d, b, :n])
            else:
                e = rel_l2(got[what][b, :n, d], ref[what][b, :n, d])
            errs.append(e)
    return worst_of(errs)


def split_saved(saved):
    """saved (B, T, 2, 240) -> gates, c, h"""
    return {"gates": saved[..., :G], "c": saved[..., G:G + H], "h": saved[..., G + H:]}
