"""Torch-tensor wrappers over the C ABI.  PyTorch is only the container for device memory and the
stream; every computation below is a liblasr.so (HIP, gfx950) call.  Tensors must live on the GPU:
there is no CPU path."""
from __future__ import annotations

import ctypes
import math
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import BF16, F32, call

ACT = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "swish": _lib.ACT_SWISH}


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError("activations must be float32 or bfloat16, got %s" % t.dtype)


def torch_dtype(code: int):
    return torch.float32 if code == F32 else torch.bfloat16


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.LasrError("liblasr ops need GPU tensors (got a %s tensor); there is no CPU fallback" % t.device)
    if not t.is_contiguous():
        raise ValueError("liblasr ops need contiguous tensors")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ---------------------------------------------------------------------------------- features
def mel_num_frames(n_samples: int) -> int:
    return int(_lib.load().lasr_mel_num_frames(n_samples))


class DeviceDither:
    """``y += 1e-5 * randn_like(y)`` (data_module.py:155) drawn inside the mel kernel: Philox keyed by ``seed``, counter =
    (sample / 4, utterance, step); ``step`` is a device scalar every mel call increments (a replayed graph draws fresh noise)."""

    def __init__(self, seed: int, device):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.step = torch.zeros(1, dtype=torch.int64, device=device)

    def noise(self, B: int, L: int) -> torch.Tensor:
        """the (B, L) N(0,1) noise the NEXT mel call draws (verification)"""
        out = torch.empty(B, L, dtype=torch.float32, device=self.step.device)
        call("lasr_dither_noise", self.seed, _p(self.step), B, L, _p(out), _stream())
        return out


def wave_src(wave: torch.Tensor, dither=None, pitch: int = 0) -> "_lib.WaveSrc":
    """lasr_wave_src for a (B, L) float32 or int16 (PCM) waveform tensor; dither: None | (B, L) f32 noise | DeviceDither;
    pitch: elements between rows when the rows are wider than the L the call is made with (0: L)"""
    if wave.dtype == torch.float32:
        wd = _lib.WAVE_F32
    elif wave.dtype == torch.int16:
        wd = _lib.WAVE_PCM16
    else:
        raise TypeError("waveforms must be float32 or int16 PCM, got %s" % wave.dtype)
    if isinstance(dither, DeviceDither):
        return _lib.WaveSrc(_p(wave), wd, None, dither.seed, _p(dither.step), int(pitch))
    if dither is not None and (dither.dtype != torch.float32 or tuple(dither.shape) != tuple(wave.shape)):
        raise TypeError("dither noise must be a float32 tensor of the waveform's shape")
    return _lib.WaveSrc(_p(wave), wd, _p(dither), 0, None, int(pitch))


def mel(wave: torch.Tensor, sample_lens: Optional[torch.Tensor] = None, dither=None,
        aug: Optional[torch.Tensor] = None, normalize: bool = True, dtype=torch.float32, want_bft: bool = True,
        want_btf: bool = True, out_btf: Optional[torch.Tensor] = None, out_pct: Optional[torch.Tensor] = None,
        logical_len: Optional[int] = None):
    """wave (B, L) f32 or int16 PCM -> (feats_bft (B,64,T) f32 | None, feats_btf (B,T,64) dtype | None, frames (B) i32, pct (B) f32).
    dither: None, a (B, L) N(0,1) tensor, or a DeviceDither (noise generated inside the kernel).
    logical_len: the batch's longest utterance when the rows of `wave` are wider than that (a loader's static row pitch): T = the
    frames of `logical_len` samples - the reference's pad-to-longest (data_module.py:222-248) - not of the row width."""
    B, P = wave.shape
    L = int(logical_len) if logical_len is not None else P
    if not 0 < L <= P:
        raise ValueError("logical_len %s outside the rows' width %d" % (logical_len, P))
    T = mel_num_frames(L)
    dev = wave.device
    bft = torch.empty(B, 64, T, dtype=torch.float32, device=dev) if want_bft else None
    btf = None
    if out_btf is not None:
        if tuple(out_btf.shape) != (B, T, 64) or out_btf.dtype != dtype or not out_btf.is_contiguous():
            raise ValueError("out_btf must be a contiguous (%d, %d, 64) %s tensor" % (B, T, dtype))
        btf = out_btf
    elif want_btf:
        btf = torch.empty(B, T, 64, dtype=dtype, device=dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    pct = out_pct if out_pct is not None else torch.empty(B, dtype=torch.float32, device=dev)
    nb = _lib.load().lasr_mel_workspace_bytes(B, T)
    ws = _ws(nb, dev)
    src = wave_src(wave, dither, P if P != L else 0)
    call("lasr_mel_fwd_src", _lib.C.byref(src), _p(sample_lens), _p(aug), B, L, int(normalize), _p(bft), _p(btf),
         F32 if dtype == torch.float32 else BF16, _p(frames), _p(pct), _p(ws), nb, _stream())
    return bft, btf, frames, pct


def bct_to_btc(x: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    B, Cc, T = x.shape
    out = torch.empty(B, T, Cc, dtype=dtype, device=x.device)
    call("lasr_bct_to_btc", _p(x), _p(out), _dt(out), B, Cc, T, _stream())
    return out


def btc_to_bct(x: torch.Tensor) -> torch.Tensor:
    B, T, Cc = x.shape
    out = torch.empty(B, Cc, T, dtype=torch.float32, device=x.device)
    call("lasr_btc_to_bct", _p(x), _dt(x), _p(out), B, Cc, T, _stream())
    return out


def mask_lengths(pct: torch.Tensor, T: int) -> torch.Tensor:
    lens = torch.empty(pct.numel(), dtype=torch.int32, device=pct.device)
    call("lasr_mask_lengths", _p(pct), pct.numel(), T, _p(lens), _stream())
    return lens


# ---------------------------------------------------------------------------------- conv pieces
def dwconv(x: torch.Tensor, w: torch.Tensor, stride: int = 1, flip: bool = False,
           addend: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B][T][C], w (C, k) or (C,1,k) f32."""
    B, Tin, Cc = x.shape
    k = w.shape[-1]
    Tout = (Tin + 2 * (k // 2) - k) // stride + 1
    y = torch.empty(B, Tout, Cc, dtype=x.dtype, device=x.device)
    call("lasr_dwconv_fwd", _p(x), _p(w), _p(addend), _p(y), _dt(x), B, Tin, Cc, k, stride, int(flip), _stream())
    return y


def dwconv_wgrad(x: torch.Tensor, dy: torch.Tensor, k: int, stride: int = 1) -> torch.Tensor:
    B, Tin, Cc = x.shape
    dw = torch.empty(Cc, k, dtype=torch.float32, device=x.device)
    nb = _lib.load().lasr_dwconv_wgrad_workspace_bytes(B, dy.shape[1], Cc, k)
    ws = _ws(nb, x.device)
    call("lasr_dwconv_wgrad", _p(x), _p(dy), _p(dw), _dt(x), B, Tin, Cc, k, stride, _p(ws), nb, _stream())
    return dw


def gemm(A: torch.Tensor, Bm: torch.Tensor, M: int, N: int, K: int, transA: bool = False, transB: bool = False,
         bias: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None,
         row_lens: Optional[torch.Tensor] = None, rows_per_seq: int = 0, want_stats: bool = False, split_k: int = 1,
         out_dtype=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    out_dtype = out_dtype or A.dtype
    Cm = torch.empty(M, N, dtype=out_dtype, device=A.device)
    stats = torch.empty(2 * N, dtype=torch.float32, device=A.device) if want_stats else None
    nb = _lib.load().lasr_gemm_workspace_bytes(M, N, split_k, int(want_stats))
    ws = _ws(nb, A.device)
    call("lasr_gemm", _p(A), _p(Bm), _p(Cm), _dt(A), _dt(Cm), M, N, K, int(transA), int(transB), _p(bias), _p(addend),
         _p(row_lens), rows_per_seq, _p(stats), split_k, _p(ws), nb, _stream())
    return Cm, stats


def gemm_ld(A, lda, Bm, ldb, M, N, K, transA=False, transB=False, split_k: int = 1, out_dtype=None, ldc: int = 0):
    """lasr_gemm_ld: operands given as flat/padded buffers with explicit pitches; returns C (M, ldc or N)."""
    out_dtype = out_dtype or A.dtype
    Cm = torch.empty(M, ldc or N, dtype=out_dtype, device=A.device)
    nb = _lib.load().lasr_gemm_workspace_bytes(M, N, split_k, 0)
    ws = _ws(nb, A.device)
    call("lasr_gemm_ld", _p(A), lda, _p(Bm), ldb, _p(Cm), ldc, _dt(A), _dt(Cm), M, N, K, int(transA), int(transB), None, split_k,
         _p(ws), nb, _stream())
    return Cm


class _ReduceDesc(_lib.C.Structure):
    _fields_ = [("partials", _lib.C.c_void_p), ("out", _lib.C.c_void_p), ("n", _lib.C.c_int64), ("n_partials", _lib.C.c_int32)]


def reduce_many(segments):
    """segments: list of (partials (P_i, n_i) f32, out (n_i,) f32): out_i = partials_i.sum(0), one launch (<= 64)."""
    descs = (_ReduceDesc * len(segments))()
    for i, (pt, out) in enumerate(segments):
        descs[i].partials, descs[i].out, descs[i].n, descs[i].n_partials = _p(pt), _p(out), out.numel(), pt.shape[0]
    call("lasr_reduce_many", descs, len(segments), _stream())


def wgrad_multi(dys, xs, split_k: int = 4):
    """The 1x1 weight gradients dW_i = dy_i^T x_i of several layers in ONE split-K launch + ONE reduction
    (lasr_gemm_multi_split_partials + lasr_reduce_many).  dys[i] (rows, co_i), xs[i] (rows, ci_i) bf16."""
    n = len(dys)
    dev = dys[0].device
    probs = (_GemmProblem * n)()
    slabs = (_lib.C.c_void_p * n)()
    splits = (_lib.C.c_int * n)()
    outs, bufs = [], []
    for i in range(n):
        rows, co = dys[i].shape
        ci = xs[i].shape[1]
        out = torch.empty(co, ci, dtype=torch.float32, device=dev)
        buf = torch.empty(split_k, co * ci, dtype=torch.float32, device=dev)
        probs[i].A, probs[i].B, probs[i].C = _p(dys[i]), _p(xs[i]), _p(out)
        probs[i].M, probs[i].N, probs[i].K = co, ci, rows
        probs[i].bias = None; probs[i].row_lens = None; probs[i].rows_per_seq = 0; probs[i].stats = None
        slabs[i] = _p(buf)
        outs.append(out); bufs.append(buf)
    call("lasr_gemm_multi_split_partials", probs, n, split_k, slabs, splits, _stream())
    reduce_many([(bufs[i][:splits[i]], outs[i].view(-1)) for i in range(n)])
    return outs


def dwconv_bwd_fused(x: torch.Tensor, dy: torch.Tensor, w: torch.Tensor, addend: Optional[torch.Tensor] = None):
    """Depthwise backward of a stride-1 layer in one launch: (dW (C, k) f32, dx (B, T, C)) from x, dy (B, T, C) and the taps
    w (C, 1, k) / (C, k) f32 (lasr_dwconv_bwd_fused + lasr_reduce_many)."""
    B, T, Cc = x.shape
    k = w.shape[-1]
    dx = torch.empty_like(dy)
    nb = _lib.load().lasr_dwconv_wgrad_workspace_bytes(B, T, Cc, k)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    npart = _lib.C.c_int(0)
    call("lasr_dwconv_bwd_fused", _p(x), _p(dy), _p(w), _p(addend), _p(dx), _dt(x), B, T, Cc, k, _p(ws), nb, _lib.C.byref(npart), _stream())
    dw = torch.empty(Cc, k, dtype=torch.float32, device=x.device)
    reduce_many([(ws.view(torch.float32)[:npart.value * Cc * k].view(npart.value, Cc * k), dw.view(-1))])
    return dw, dx


class _FoldDesc(_lib.C.Structure):
    _fields_ = [("w", _lib.C.c_void_p), ("w_res", _lib.C.c_void_p), ("coef", _lib.C.c_void_p), ("coef2", _lib.C.c_void_p),
                ("w_out", _lib.C.c_void_p), ("bias_out", _lib.C.c_void_p), ("co", _lib.C.c_int64), ("ci", _lib.C.c_int64)]


def fold_bn_weights(w: torch.Tensor, coef: torch.Tensor, w_res: Optional[torch.Tensor] = None, coef2: Optional[torch.Tensor] = None):
    """Eval-mode BN folded into 1x1 conv weights: ([a W | a2 Wr] bf16 (co, ci (+ci)), b (+ b2) f32 (co)); coef = [a | b]."""
    co, ci = w.shape[0], w.shape[1]
    wout = torch.empty(co, ci * (2 if w_res is not None else 1), dtype=torch.bfloat16, device=w.device)
    bias = torch.empty(co, dtype=torch.float32, device=w.device)
    d = (_FoldDesc * 1)()
    d[0].w, d[0].w_res, d[0].coef, d[0].coef2 = _p(w), _p(w_res), _p(coef), _p(coef2)
    d[0].w_out, d[0].bias_out, d[0].co, d[0].ci = _p(wout), _p(bias), co, ci
    call("lasr_fold_bn_weights_many", d, 1, _stream())
    return wout, bias


def gemm_dual(a1: torch.Tensor, a2: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, row_lens: Optional[torch.Tensor] = None,
              rows_per_seq: int = 0, act: str = "relu") -> torch.Tensor:
    """act([a1 (rows past row_lens zeroed) | a2] @ w.T + bias): a1 (M, K1), a2 (M, K2), w (N, K1 + K2) bf16 -> (M, N) bf16."""
    M, K1 = a1.shape
    K2 = a2.shape[1]
    N = w.shape[0]
    out = torch.empty(M, N, dtype=torch.bfloat16, device=a1.device)
    call("lasr_gemm_dual", _p(a1), K1, _p(a2), K2, _p(w), _p(bias), _p(out), M, N, _p(row_lens), rows_per_seq, ACT[act], _stream())
    return out


def bn_finalize(stats, gamma, beta, running_mean, running_var, n_rows: int, eps: float = 1e-3, momentum: float = 0.1,
                training: bool = True):
    Cc = gamma.numel()
    coef = torch.empty(2 * Cc, dtype=torch.float32, device=gamma.device)
    saved = torch.empty(2 * Cc, dtype=torch.float32, device=gamma.device)
    call("lasr_bn_finalize", _p(stats), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(coef), _p(saved), Cc,
         n_rows, eps, momentum, int(training), _stream())
    return coef, saved


class _GemmProblem(_lib.C.Structure):
    _fields_ = [("A", _lib.C.c_void_p), ("B", _lib.C.c_void_p), ("C", _lib.C.c_void_p), ("M", _lib.C.c_int64), ("N", _lib.C.c_int64),
                ("K", _lib.C.c_int64), ("bias", _lib.C.c_void_p), ("row_lens", _lib.C.c_void_p), ("rows_per_seq", _lib.C.c_int64),
                ("stats", _lib.C.c_void_p)]


class _BnBranch(_lib.C.Structure):
    _fields_ = [("partials", _lib.C.c_void_p), ("n_partials", _lib.C.c_int), ("gamma", _lib.C.c_void_p), ("beta", _lib.C.c_void_p),
                ("running_mean", _lib.C.c_void_p), ("running_var", _lib.C.c_void_p), ("coef", _lib.C.c_void_p),
                ("saved", _lib.C.c_void_p), ("stats", _lib.C.c_void_p)]


def gemm_bn_fused(xs, ws_, bns, row_lens=None, rows_per_seq: int = 0, eps: float = 1e-3, momentum: float = 0.1):
    """A unit's 1x1 convolutions (1 or 2 problems: y_i = x_i @ w_i^T, the first optionally row-masked) with
    training-mode BN coefficients from the epilogue's partial sums in one reduce+finalize launch.
    bns[i] = (gamma, beta, running_mean, running_var).  Returns ([y_i], [coef_i], [saved_i], [stats_i])."""
    n = len(xs)
    dev = xs[0].device
    M = xs[0].shape[0]
    probs = (_GemmProblem * 2)()
    ys, coefs, saveds, stats = [], [], [], []
    for i in range(n):
        N, K = ws_[i].shape
        y = torch.empty(M, N, dtype=xs[i].dtype, device=dev)
        st = torch.empty(2 * N, dtype=torch.float32, device=dev)
        probs[i].A, probs[i].B, probs[i].C = _p(xs[i]), _p(ws_[i]), _p(y)
        probs[i].M, probs[i].N, probs[i].K = M, N, K
        probs[i].bias = None
        probs[i].row_lens = _p(row_lens) if (i == 0 and row_lens is not None) else None
        probs[i].rows_per_seq = rows_per_seq if i == 0 else 0
        probs[i].stats = _p(st)
        ys.append(y); stats.append(st)
    nb = sum(_lib.load().lasr_gemm_workspace_bytes(M, ws_[i].shape[0], 1, 1) for i in range(n))
    wsb = _ws(nb, dev)
    parts = (_lib.C.c_void_p * 2)()
    tiles = (_lib.C.c_int * 2)()
    call("lasr_gemm_batch_partials", probs, n, _dt(xs[0]), _dt(xs[0]), 0, 0, _p(wsb), wsb.numel(), parts, tiles, _stream())
    brs = (_BnBranch * 2)()
    for i in range(n):
        N = ws_[i].shape[0]
        g, b, rm, rv = bns[i]
        coef = torch.empty(2 * N, dtype=torch.float32, device=dev)
        saved = torch.empty(2 * N, dtype=torch.float32, device=dev)
        brs[i].partials, brs[i].n_partials = parts[i], tiles[i]
        brs[i].gamma, brs[i].beta, brs[i].running_mean, brs[i].running_var = _p(g), _p(b), _p(rm), _p(rv)
        brs[i].coef, brs[i].saved, brs[i].stats = _p(coef), _p(saved), _p(stats[i])
        coefs.append(coef); saveds.append(saved)
    call("lasr_bn_finalize_partials", brs, n, ws_[0].shape[0], M, eps, momentum, _stream())
    return ys, coefs, saveds, stats


def _bn_tail(y, main, res=None, act: str = "relu", **fields) -> _lib.BnTail:
    """lasr_bn_tail (include/lasr.h) from tensors.  y (B,T,C): the main branch's pre-BN tensor, which also fixes dtype and shape;
    main / res: the other lasr_bn_side fields by name (coef, saved, gamma, sums, dy, ...), res with its own y, or None / y None
    without a residual branch; fields: dout, se_scale, se_grad, row_lens.  A None tensor is NULL.  The record holds the tensors,
    so they live as long as it does."""
    B, T, Cc = y.shape
    t = _lib.BnTail(dtype=_dt(y), act=ACT[act], B=B, T=T, C=Cc)
    t.tensors = []
    for rec, named in ((t.main, dict(main, y=y)), (t.res, res if res and res.get("y") is not None else {}), (t, fields)):
        for name, tensor in named.items():
            setattr(rec, name, _p(tensor))
            t.tensors.append(tensor)
    return t


def bn_act(y, coef, y2=None, coef2=None, se_scale=None, act: str = "relu") -> torch.Tensor:
    out = torch.empty_like(y)
    tail = _bn_tail(y, dict(coef=coef), dict(y=y2, coef=coef2), act, se_scale=se_scale)
    call("lasr_bn_act_fwd", ctypes.byref(tail), _p(out), _stream())
    return out


def se_fwd(y, coef, W1, W2):
    """SELayer forward on the pre-BN tensor y (B,T,C) (models/QuartNetContextSE.py:8-23): the squeeze is taken through the BN
    coefficients coef [2][C] (mean_T(BN(y)) = a * mean_T(y) + b).  -> (ysum (B,C), pooled (B,C), hidden (B,C/8), scale (B,C)), f32."""
    B, T, Cc = y.shape
    dev = y.device
    ysum = torch.empty(B, Cc, dtype=torch.float32, device=dev)
    pooled = torch.empty(B, Cc, dtype=torch.float32, device=dev)
    hidden = torch.empty(B, Cc // 8, dtype=torch.float32, device=dev)
    scale = torch.empty(B, Cc, dtype=torch.float32, device=dev)
    call("lasr_seqsum", _p(y), _dt(y), B, T, Cc, _p(ysum), _stream())
    call("lasr_se_fwd", _p(ysum), _p(coef), _p(W1), _p(W2), B, T, Cc, _p(pooled), _p(hidden), _p(scale), _stream())
    return ysum, pooled, hidden, scale


def se_bwd(dout, y, coef, scale, hidden, pooled, W1, W2, y2=None, coef2=None, act: str = "relu"):
    """Backward of the SE branch of out = act(BN(y) * scale + BN2(y2)): -> (seg (B,C) = d(loss)/d(BN output) through the pooled
    mean, dW1 (C/8,C), dW2 (C,C/8))."""
    B, T, Cc = y.shape
    dev = y.device
    seg = torch.empty(B, Cc, dtype=torch.float32, device=dev)
    dW1 = torch.empty(Cc // 8, Cc, dtype=torch.float32, device=dev)
    dW2 = torch.empty(Cc, Cc // 8, dtype=torch.float32, device=dev)
    nb = int(_lib.load().lasr_se_bwd_workspace_bytes(B, Cc))
    ws = _ws(nb, dev)
    tail = _bn_tail(y, dict(coef=coef), dict(y=y2, coef=coef2), act, dout=dout, se_scale=scale)
    se = _lib.SeSide(hidden=_p(hidden), pooled=_p(pooled), W1=_p(W1), W2=_p(W2), seg=_p(seg), dW1=_p(dW1), dW2=_p(dW2))
    call("lasr_se_bwd", ctypes.byref(tail), ctypes.byref(se), _p(ws), nb, _stream())
    return seg, dW1, dW2


def bn_act_bwd(dout, y, coef, saved, gamma, y2=None, coef2=None, saved2=None, gamma2=None, se_scale=None, se_grad=None,
               row_lens=None, act: str = "relu", fused: bool = False):
    """Returns (dy, dy2, dgamma, dbeta, dgamma2, dbeta2).  fused: pass 2 reduces pass 1's partial sums itself."""
    B, T, Cc = y.shape
    dev = y.device
    sums = torch.empty(2 * Cc, dtype=torch.float32, device=dev)
    sums2 = torch.empty(2 * Cc, dtype=torch.float32, device=dev)
    nb = max(_lib.load().lasr_bn_bwd_workspace_bytes(B, T, Cc), _lib.load().lasr_bn_bwd_apply_workspace_bytes(Cc))
    ws = _ws(nb, dev)
    if fused:
        sums = sums2 = None
    dy = torch.empty_like(y)
    dy2 = torch.empty_like(y) if y2 is not None else None
    dg, db = (torch.empty(Cc, dtype=torch.float32, device=dev) for _ in range(2))
    dg2, db2 = ((torch.empty(Cc, dtype=torch.float32, device=dev) for _ in range(2)) if y2 is not None else (None, None))
    tail = _bn_tail(y, dict(coef=coef, saved=saved, gamma=gamma, sums=sums, dy=dy, dgamma=dg, dbeta=db),
                    dict(y=y2, coef=coef2, saved=saved2, gamma=gamma2, sums=sums2, dy=dy2, dgamma=dg2, dbeta=db2), act,
                    dout=dout, se_scale=se_scale, se_grad=se_grad, row_lens=row_lens)
    call("lasr_bn_act_bwd_stats", ctypes.byref(tail), _p(ws), nb, _stream())
    call("lasr_bn_act_bwd_apply", ctypes.byref(tail), _p(ws), ws.numel(), _stream())
    return dy, dy2, dg, db, dg2, db2


# ---------------------------------------------------------------------------------- head + loss
def log_softmax(logits: torch.Tensor, want_argmax: bool = True):
    shp = logits.shape
    Cc = shp[-1]
    N = logits.numel() // Cc
    out = torch.empty_like(logits)
    am = torch.empty(shp[:-1], dtype=torch.int32, device=logits.device) if want_argmax else None
    call("lasr_log_softmax", _p(logits), _p(out), _p(am), N, Cc, _stream())
    return out, am


CTC_MAX_LABELS = 2047   # LASR_CTC_MAX_LABELS (include/lasr.h): the longest label sequence the CTC kernels take


def ctc_loss(logp: torch.Tensor, targets: torch.Tensor, in_lens: torch.Tensor, tgt_lens: torch.Tensor, blank: int,
             want_grad: bool = True, gscale: Optional[torch.Tensor] = None):
    """logp (B,T,C) f32 -> (nll (B), grad (B,T,C) | None); grad is torch's CTCLoss backward for grad_output=gscale.
    targets (B, S) with S <= CTC_MAX_LABELS."""
    B, T, Cc = logp.shape
    S = targets.shape[1] if targets.dim() == 2 else 0
    if S > CTC_MAX_LABELS:
        raise ValueError("ctc_loss: targets are %d labels wide; the CTC kernels take at most %d" % (S, CTC_MAX_LABELS))
    nll = torch.empty(B, dtype=torch.float32, device=logp.device)
    grad = torch.empty_like(logp) if want_grad else None
    nb = _lib.load().lasr_ctc_workspace_bytes(B, T, max(S, 1))
    ws = _ws(nb, logp.device)
    call("lasr_ctc_loss", _p(logp), _p(targets), _p(in_lens), _p(tgt_lens), B, T, Cc, max(S, 1), blank, _p(nll), _p(grad),
         _p(gscale), _p(ws), nb, _stream())
    return nll, grad


class CtcAlignment(NamedTuple):
    score: torch.Tensor          # (B,) f32 Viterbi log-probability, -inf when no alignment exists
    frame_state: torch.Tensor    # (B, T) i32 lattice state 0..2S of every frame, -1 past in_lens / infeasible
    frame_logp: torch.Tensor     # (B, T) f32 log-prob of that state's class, 0 where frame_state is -1
    label_start: torch.Tensor    # (B, S) i32 first frame of label i, -1 for i >= tgt_lens / infeasible
    label_end: torch.Tensor      # (B, S) i32 one past its last frame


def ctc_align(logp: torch.Tensor, targets: torch.Tensor, in_lens: Optional[torch.Tensor], tgt_lens: torch.Tensor,
              blank: int) -> CtcAlignment:
    """CTC forced alignment (Viterbi path of the ctc_loss lattice, include/lasr.h lasr_ctc_align) of logp (B,T,C) f32 to targets
    (B,S) i64, S <= CTC_MAX_LABELS; in_lens (B) i32 or None (= T), tgt_lens (B) i32.  One launch, nothing synchronised - except
    that the labels inside tgt_lens are checked on the host first (skipped while the stream is being captured into a graph;
    the kernel clamps them)."""
    if logp.dim() != 3 or logp.dtype != torch.float32:
        raise ValueError("ctc_align takes (B, T, C) float32 log-probs")
    B, T, Cc = logp.shape
    if targets.dim() != 2 or targets.shape[0] != B or targets.dtype != torch.int64:
        raise ValueError("ctc_align: targets must be (B, S) int64")
    S = targets.shape[1]
    if S > CTC_MAX_LABELS:
        raise ValueError("ctc_align: targets are %d labels wide; the CTC kernels take at most %d" % (S, CTC_MAX_LABELS))
    for name, t in (("in_lens", in_lens), ("tgt_lens", tgt_lens)):
        if t is None and name == "in_lens":
            continue
        if t is None or t.shape != (B,) or t.dtype != torch.int32:
            raise ValueError("ctc_align: %s must be (B,) int32" % name)
    if B < 1 or T < 1 or not 0 <= blank < Cc or Cc < 2:
        raise ValueError("ctc_align: shape (%d, %d, %d) with blank %d" % (B, T, Cc, blank))
    if S > 0 and not (logp.is_cuda and torch.cuda.is_current_stream_capturing()):
        live = torch.arange(S, device=targets.device).unsqueeze(0) < tgt_lens.unsqueeze(1)
        bad = live & ((targets == blank) | (targets < 0) | (targets >= Cc))
        if bool(bad.any()):
            b, i = [int(v) for v in bad.nonzero()[0]]
            raise ValueError("ctc_align: targets[%d][%d] = %d is the blank or outside [0, %d)" % (b, i, int(targets[b, i]), Cc))
    nb = int(_lib.load().lasr_ctc_align_workspace_bytes(B, T, S))
    dev = logp.device
    out = CtcAlignment(torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, T, dtype=torch.int32, device=dev),
                       torch.empty(B, T, dtype=torch.float32, device=dev), torch.empty(B, S, dtype=torch.int32, device=dev),
                       torch.empty(B, S, dtype=torch.int32, device=dev))
    ws = _ws(nb, dev)
    call("lasr_ctc_align", _p(logp), _p(targets) if S else None, _p(in_lens), _p(tgt_lens), B, T, Cc, S, int(blank), _p(out.score),
         _p(out.frame_state), _p(out.frame_logp), _p(out.label_start) if S else None, _p(out.label_end) if S else None, _p(ws), nb,
         _stream())
    return out


CTC_ALIGN_LONG_MAX_LABELS = 1 << 24   # LASR_CTC_ALIGN_LONG_MAX_LABELS (include/lasr.h)
CTC_ALIGN_LONG_MAX_BAND = 8192        # LASR_CTC_ALIGN_LONG_MAX_BAND: the widest band of ctc_align_long


class CtcAlignmentLong(NamedTuple):
    score: torch.Tensor          # the fields of CtcAlignment ...
    frame_state: torch.Tensor
    frame_logp: torch.Tensor
    label_start: torch.Tensor
    label_end: torch.Tensor
    status: torch.Tensor         # (B,) i32: 0 aligned, 1 infeasible by count, 2 lost by the band
    band_lo: torch.Tensor        # (B, T) i32: the band's first state in every frame, -1 past in_lens


def ctc_align_long_period() -> int:
    """R: the band of ctc_align_long can move only at frames that are multiples of it"""
    return int(_lib.load().lasr_ctc_align_long_period())


def ctc_align_long_granule() -> int:
    """G: the band origin of ctc_align_long is a multiple of it"""
    return int(_lib.load().lasr_ctc_align_long_granule())


def ctc_align_long_band_at_least(n: int) -> Optional[int]:
    """the narrowest band ctc_align_long takes that holds at least n states (a multiple of 256 up to 4096, of 1024 up to
    CTC_ALIGN_LONG_MAX_BAND), or None when n is above the widest"""
    n = max(int(n), 256)
    band = -(-n // 256) * 256 if n <= 4096 else -(-n // 1024) * 1024
    return band if band <= CTC_ALIGN_LONG_MAX_BAND else None


def ctc_align_long(logp: torch.Tensor, targets: torch.Tensor, in_lens: Optional[torch.Tensor], tgt_lens: torch.Tensor,
                   blank: int, band: int = 4096) -> CtcAlignmentLong:
    """ctc_align for long recordings (include/lasr.h lasr_ctc_align_long): the Viterbi path inside a band of `band` states that
    follows it, so targets (B,S) may be far wider than CTC_MAX_LABELS and T * C is not bounded by 2^31.  band: a multiple of 256 up
    to 4096 or a multiple of 1024 up to CTC_ALIGN_LONG_MAX_BAND.  With band >= 2 S + 1 the result is ctc_align's bit for bit; a
    narrower band prunes - it may return a feasible path that is not the best one without any flag, or none (status 2).  One
    launch, nothing synchronised, except for the host-side label check of ctc_align (skipped during graph capture)."""
    if logp.dim() != 3 or logp.dtype != torch.float32:
        raise ValueError("ctc_align_long takes (B, T, C) float32 log-probs")
    B, T, Cc = logp.shape
    if targets.dim() != 2 or targets.shape[0] != B or targets.dtype != torch.int64:
        raise ValueError("ctc_align_long: targets must be (B, S) int64")
    S = targets.shape[1]
    if S > CTC_ALIGN_LONG_MAX_LABELS:
        raise ValueError("ctc_align_long: targets are %d labels wide; the kernel takes at most %d" % (S, CTC_ALIGN_LONG_MAX_LABELS))
    for name, t in (("in_lens", in_lens), ("tgt_lens", tgt_lens)):
        if t is None and name == "in_lens":
            continue
        if t is None or t.shape != (B,) or t.dtype != torch.int32:
            raise ValueError("ctc_align_long: %s must be (B,) int32" % name)
    if B < 1 or T < 1 or not 0 <= blank < Cc or Cc < 2:
        raise ValueError("ctc_align_long: shape (%d, %d, %d) with blank %d" % (B, T, Cc, blank))
    band = int(band)
    nb = int(_lib.load().lasr_ctc_align_long_workspace_bytes(B, T, S, band))
    if nb == 0:
        raise ValueError("ctc_align_long: band %d is not a multiple of 256 up to 4096 or of 1024 up to %d" % (band, CTC_ALIGN_LONG_MAX_BAND))
    if S > 0 and not (logp.is_cuda and torch.cuda.is_current_stream_capturing()):
        live = torch.arange(S, device=targets.device).unsqueeze(0) < tgt_lens.unsqueeze(1)
        bad = live & ((targets == blank) | (targets < 0) | (targets >= Cc))
        if bool(bad.any()):
            b, i = [int(v) for v in bad.nonzero()[0]]
            raise ValueError("ctc_align_long: targets[%d][%d] = %d is the blank or outside [0, %d)" % (b, i, int(targets[b, i]), Cc))
    dev = logp.device
    i32 = dict(dtype=torch.int32, device=dev)
    out = CtcAlignmentLong(torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, T, **i32),
                           torch.empty(B, T, dtype=torch.float32, device=dev), torch.empty(B, S, **i32), torch.empty(B, S, **i32),
                           torch.empty(B, **i32), torch.empty(B, T, **i32))
    ws = _ws(nb, dev)
    call("lasr_ctc_align_long", _p(logp), _p(targets) if S else None, _p(in_lens), _p(tgt_lens), B, T, Cc, S, int(blank), band,
         _p(out.score), _p(out.frame_state), _p(out.frame_logp), _p(out.label_start) if S else None, _p(out.label_end) if S else None,
         _p(out.status), _p(out.band_lo), _p(ws), nb, _stream())
    return out


KWS_MAX_LABELS = 64     # LASR_KWS_MAX_LABELS (include/lasr.h): the longest phrase of a keyword bank


class KeywordBank:
    """The phrases of a keyword search on the device (build_keywords): labels (sum of lengths,) i32 concatenated, offsets
    (K + 1,) i32; lengths is the host copy of the phrase lengths, max_len the longest."""

    def __init__(self, labels: torch.Tensor, offsets: torch.Tensor, lengths, n_classes: int, blank: int):
        self.labels, self.offsets = labels, offsets
        self.lengths = [int(n) for n in lengths]
        self.n_phrases, self.max_len = len(self.lengths), max(self.lengths)
        self.n_classes, self.blank = int(n_classes), int(blank)

    def __repr__(self):
        return "KeywordBank(n_phrases=%d, max_len=%d, on %s)" % (self.n_phrases, self.max_len, self.labels.device)


class KeywordHits(NamedTuple):
    n_hits: torch.Tensor         # (B, K) i32 hits of the pair; may exceed max_hits (the slots hold the first max_hits)
    hit_span: torch.Tensor       # (B, K, max_hits, 2) i32 [start frame, end frame) in time order, (-1, -1) for unwritten slots
    hit_score: torch.Tensor      # (B, K, max_hits) f32 log-likelihood ratio against the greedy path over the span, 0 if unwritten
    best_score: torch.Tensor     # (B, K) f32 the best end score whatever the threshold, -inf when the phrase does not fit
    best_span: torch.Tensor      # (B, K, 2) i32 its span, (-1, -1) with -inf


def build_keywords(phrases_ids, *, n_classes: int, blank: int, device="cuda") -> KeywordBank:
    """The bank of a keyword search from `phrases_ids`, a non-empty list of label-id lists (1..KWS_MAX_LABELS ids in
    [0, n_classes), none the blank; duplicates are fine), uploaded to `device`.  A bad phrase raises ValueError naming its index,
    before anything is uploaded."""
    phrases = [[int(c) for c in p] for p in phrases_ids]
    if not phrases:
        raise ValueError("build_keywords: no phrase")
    if not 0 <= int(blank) < int(n_classes):
        raise ValueError("build_keywords: blank %d outside [0, %d)" % (blank, n_classes))
    for i, p in enumerate(phrases):
        if not p:
            raise ValueError("build_keywords: phrase %d is empty" % i)
        if len(p) > KWS_MAX_LABELS:
            raise ValueError("build_keywords: phrase %d has %d labels; a keyword takes at most %d" % (i, len(p), KWS_MAX_LABELS))
        for c in p:
            if c == blank or not 0 <= c < n_classes:
                raise ValueError("build_keywords: phrase %d holds the label %d: the blank or outside [0, %d)" % (i, c, n_classes))
    lengths = [len(p) for p in phrases]
    offsets = np.zeros(len(phrases) + 1, dtype=np.int32)
    np.cumsum(lengths, out=offsets[1:])
    labels = np.asarray([c for p in phrases for c in p], dtype=np.int32)
    return KeywordBank(torch.from_numpy(labels).to(device), torch.from_numpy(offsets).to(device), lengths, n_classes, blank)


def ctc_keyword_search(logp: torch.Tensor, lens: Optional[torch.Tensor], blank: int, bank: KeywordBank, threshold: float = -2.0,
                       max_hits: int = 8) -> KeywordHits:
    """CTC keyword search (include/lasr.h lasr_ctc_kws): where in each row of logp (B, T, C) f32 is each phrase of `bank` said.
    lens (B) i32 or None (= T).  A hit's score is the log-likelihood ratio of the phrase's best path against the greedy path
    over the same frames (<= 0); a span is a hit when its score is at least threshold * (labels of the phrase), overlapping
    spans of one phrase keep the best.  threshold in (-1e6, 0], in natural-log units per label; the default -2.0 is a
    starting value: nobody has tuned it on a trained model (keyword_scores of AsrTranslator shows what a recording gives).  One
    launch (two for a large vocabulary), nothing synchronised."""
    if not isinstance(bank, KeywordBank):
        raise TypeError("bank must be a KeywordBank (ops.build_keywords)")
    if logp.dim() != 3 or logp.dtype != torch.float32:
        raise ValueError("ctc_keyword_search takes (B, T, C) float32 log-probs")
    B, T, Cc = logp.shape
    if lens is not None and (lens.shape != (B,) or lens.dtype != torch.int32):
        raise ValueError("ctc_keyword_search: lens must be (B,) int32")
    if B < 1 or T < 1 or Cc < 2 or not 0 <= blank < Cc:
        raise ValueError("ctc_keyword_search: shape (%d, %d, %d) with blank %d" % (B, T, Cc, blank))
    if int(max_hits) < 1:
        raise ValueError("ctc_keyword_search: max_hits must be at least 1")
    if bank.n_classes != Cc or bank.blank != blank:
        raise ValueError("the keyword bank was built for %d classes with blank %d; the log-probs have %d classes, blank %d"
                         % (bank.n_classes, bank.blank, Cc, blank))
    if logp.is_cuda and bank.labels.device != logp.device:
        raise ValueError("the keyword bank is on %s, the log-probs on %s" % (bank.labels.device, logp.device))
    K, dev = bank.n_phrases, logp.device
    ptrs = [_p(logp), _p(lens), _p(bank.labels), _p(bank.offsets)]      # CPU tensors are refused here, before anything is allocated
    out = KeywordHits(torch.empty(B, K, dtype=torch.int32, device=dev), torch.empty(B, K, int(max_hits), 2, dtype=torch.int32, device=dev),
                      torch.empty(B, K, int(max_hits), dtype=torch.float32, device=dev), torch.empty(B, K, dtype=torch.float32, device=dev),
                      torch.empty(B, K, 2, dtype=torch.int32, device=dev))
    nb = int(_lib.load().lasr_ctc_kws_workspace_bytes(B, T, K))
    ws = _ws(nb, dev)
    call("lasr_ctc_kws", ptrs[0], ptrs[1], B, T, Cc, int(blank), ptrs[2], ptrs[3], K, bank.max_len, float(threshold), int(max_hits),
         _p(out.n_hits), _p(out.hit_span), _p(out.hit_score), _p(out.best_score), _p(out.best_span), _p(ws), nb, _stream())
    return out


def greedy_decode(ids: torch.Tensor, lens: Optional[torch.Tensor], blank: int):
    B, T = ids.shape
    tokens = torch.empty(B, T, dtype=torch.int32, device=ids.device)
    n = torch.empty(B, dtype=torch.int32, device=ids.device)
    call("lasr_greedy_decode", _p(ids), _p(lens), B, T, blank, _p(tokens), _p(n), _stream())
    return tokens, n


class GreedyConfidence(NamedTuple):
    tokens: torch.Tensor         # (B, T) i32 collapsed classes, -1 from n_tokens on
    n_tokens: torch.Tensor       # (B,) i32
    tok_start: torch.Tensor      # (B, T) i32 first frame of token i's run, -1 from n_tokens on
    tok_end: torch.Tensor        # (B, T) i32 one past its last frame
    tok_mean: torch.Tensor       # (B, T) f32 mean of the frame maxima over the run, 0 from n_tokens on
    tok_min: torch.Tensor        # (B, T) f32 their minimum
    utt_sum: torch.Tensor        # (B, 2) f64 sum of the frame maxima over [all frames, frames whose argmax is a label]
    n_nonblank: torch.Tensor     # (B,) i32 frames whose argmax is a label
    conf: torch.Tensor           # (B, 2) f32 [reference confidence, the same over label frames only]; smaller = more confident


def greedy_confidence_frame_tile() -> int:
    """frames the collapse of greedy_confidence takes per step (the sizes its tests sit at)"""
    return int(_lib.load().lasr_greedy_confidence_frame_tile())


def greedy_confidence_narrow_classes() -> int:
    """the largest class count whose rows share a wave in greedy_confidence's row pass"""
    return int(_lib.load().lasr_greedy_confidence_narrow_classes())


def greedy_confidence(logp: torch.Tensor, lens: Optional[torch.Tensor], blank: int) -> GreedyConfidence:
    """Greedy CTC decode of logp (B, T, C) f32 with token spans and confidences (include/lasr.h lasr_greedy_confidence), lens
    (B) i32 or None (= T).  Two launches, nothing synchronised; outputs as in GreedyConfidence."""
    if logp.dim() != 3 or logp.dtype != torch.float32:
        raise ValueError("greedy_confidence takes (B, T, C) float32 log-probs")
    B, T, Cc = logp.shape
    if lens is not None and (lens.shape != (B,) or lens.dtype != torch.int32):
        raise ValueError("greedy_confidence: lens must be (B,) int32")
    dev = logp.device
    ptrs = [_p(logp), _p(lens)]                                         # CPU tensors are refused here, before anything is allocated
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out = GreedyConfidence(torch.empty(B, T, **i32), torch.empty(B, **i32), torch.empty(B, T, **i32), torch.empty(B, T, **i32),
                           torch.empty(B, T, **f32), torch.empty(B, T, **f32), torch.empty(B, 2, dtype=torch.float64, device=dev),
                           torch.empty(B, **i32), torch.empty(B, 2, **f32))
    nb = int(_lib.load().lasr_greedy_confidence_workspace_bytes(B, T, Cc))
    ws = _ws(nb, dev)
    call("lasr_greedy_confidence", ptrs[0], ptrs[1], B, T, Cc, int(blank), _p(out.tokens), _p(out.n_tokens), _p(out.tok_start),
         _p(out.tok_end), _p(out.tok_mean), _p(out.tok_min), _p(out.utt_sum), _p(out.n_nonblank), _p(out.conf), _p(ws), nb, _stream())
    return out


def hyp_neg_logprob(logp: torch.Tensor, lens: Optional[torch.Tensor], tokens: torch.Tensor, n_tokens: torch.Tensor,
                    blank: int, max_tokens: Optional[int] = None) -> torch.Tensor:
    """The "posterior" confidence of a hypothesis: ctc_loss of logp (B, T, C) against each utterance's own tokens (B, T) i32 /
    n_tokens (B) i32 (as greedy_confidence writes them), i.e. minus the log of the total probability of ALL its alignments,
    divided by (Tb + 1e-6): per frame, comparable with GreedyConfidence.conf[:, 0] under one threshold.  An empty hypothesis
    scores -sum_t logp[t][blank] / (Tb + 1e-6).  max_tokens: the largest n_tokens when the caller knows it (a narrower label
    matrix; the result is the same); hypotheses of more than CTC_MAX_LABELS tokens are not supported.  Returns (B,) f32;
    nothing synchronised."""
    B, T, _ = logp.shape
    if lens is None:
        lens = torch.full((B,), T, dtype=torch.int32, device=logp.device)
    S = min(T if max_tokens is None else int(max_tokens), T, CTC_MAX_LABELS)
    # slots past n_tokens hold -1: the loss reads only the first n_tokens labels of a row, so any valid label does there
    tg = tokens[:, :max(S, 1)].clamp(min=0).to(torch.int64).contiguous()
    nll, _ = ctc_loss(logp, tg, lens, n_tokens.contiguous(), int(blank), want_grad=False)
    return nll / (lens.clamp(0, T).to(torch.float32) + 1e-6)


CTC_BEAM_MAX_WIDTH = 128     # lasr_ctc_beam_decode's supported range (include/lasr.h)
CTC_BEAM_MAX_TOP_N = 64
CTC_BEAM_MAX_CLASSES = 8192


def _beam_args(logp, lens, blank, beam_width, cutoff_top_n, cutoff_prob, n_best, who):
    """The checks both beam decoders make (`who` names the caller).  Returns (B, T, C, cutoff_top_n clamped to C)."""
    if logp.dtype != torch.float32 or logp.dim() != 3:
        raise TypeError("%s takes (B, T, C) float32 log-probs" % who)
    B, T, Cc = logp.shape
    cutoff_top_n = min(int(cutoff_top_n), Cc) if Cc >= 1 else int(cutoff_top_n)    # above C it acts as C
    if not 1 <= beam_width <= CTC_BEAM_MAX_WIDTH:
        raise ValueError("beam_width %d outside 1..%d" % (beam_width, CTC_BEAM_MAX_WIDTH))
    if not 1 <= cutoff_top_n <= CTC_BEAM_MAX_TOP_N:
        raise ValueError("cutoff_top_n %d outside 1..%d" % (cutoff_top_n, CTC_BEAM_MAX_TOP_N))
    if not 1 <= Cc <= CTC_BEAM_MAX_CLASSES:
        raise ValueError("%d classes: the beam decoder takes at most %d" % (Cc, CTC_BEAM_MAX_CLASSES))
    if not 1 <= n_best <= beam_width:
        raise ValueError("n_best %d outside 1..beam_width (%d)" % (n_best, beam_width))
    if not 0.0 < cutoff_prob <= 1.0:
        raise ValueError("cutoff_prob %r outside (0, 1]" % (cutoff_prob,))
    if not 0 <= blank < Cc:
        raise ValueError("blank %d outside [0, %d)" % (blank, Cc))
    return B, T, Cc, cutoff_top_n


def _beam_outputs(logp, n_best):
    """the (tokens, n_tokens, scores) a beam decode of logp (B, T, C) fills"""
    B, T, _ = logp.shape
    tokens = torch.empty(B, n_best, T, dtype=torch.int32, device=logp.device)
    n = torch.empty(B, n_best, dtype=torch.int32, device=logp.device)
    scores = torch.empty(B, n_best, dtype=torch.float32, device=logp.device)
    return tokens, n, scores


def ctc_beam_decode(logp: torch.Tensor, lens: Optional[torch.Tensor], blank: int, beam_width: int = 16, cutoff_top_n: int = 40,
                    cutoff_prob: float = 1.0, n_best: int = 1):
    """CTC prefix beam search (no LM) of logp (B,T,C) f32 log-probs, lens (B) i32 frames or None (= T).  Returns
    (tokens (B, n_best, T) i32, -1 past each hypothesis; n_tokens (B, n_best) i32, -1 for an empty slot; scores (B, n_best) f32
    log-probabilities, best first).  Shapes outside the kernel's range raise ValueError."""
    B, T, Cc, cutoff_top_n = _beam_args(logp, lens, blank, beam_width, cutoff_top_n, cutoff_prob, n_best, "ctc_beam_decode")
    nb = int(_lib.load().lasr_ctc_beam_workspace_bytes(B, T, Cc, beam_width, cutoff_top_n))
    if nb == 0:
        raise ValueError("ctc_beam_decode: shape (%d, %d, %d) outside the kernel's range" % (B, T, Cc))
    tokens, n, scores = _beam_outputs(logp, n_best)
    ws = _ws(nb, logp.device)
    call("lasr_ctc_beam_decode", _p(logp), _p(lens), B, T, Cc, int(blank), int(beam_width), int(cutoff_top_n), float(cutoff_prob),
         int(n_best), _p(tokens), _p(n), _p(scores), _p(ws), nb, _stream())
    return tokens, n, scores


ARPA_MAX_ORDER = 6
_E_FORMAT, _E_UNSUPPORTED, _E_IO = -4, -5, -6      # LASR_E_FORMAT / LASR_E_UNSUPPORTED / LASR_E_IO (include/lasr.h)


class ArpaNotFoundError(FileNotFoundError, NotImplementedError):
    """lm_path names no file.  Also a NotImplementedError, which is what a decoder without LM support raised for any lm_path."""


class ArpaLm:
    """An n-gram LM read from a text ARPA file (load_arpa): the device image the fused beam search reads, its order and the
    weights the decoder applies.  Character-based (is_character_based()): lasr_ctc_beam_decode_lm's image, alpha on the
    natural-log LM score, beta per emitted label.  Word-level: lasr_ctc_beam_decode_wlm's image with the lexicon of the
    n_lexicon_words words the labels can spell (n_dropped_words could not be), alpha per scored word, beta per word."""

    def __init__(self, image: torch.Tensor, order: int, char_based: bool, n_ngrams: int, vocab, alpha: float, beta: float,
                 n_lexicon_words: int = 0, n_dropped_words: int = 0):
        self.image = image
        self.order = int(order)
        self._char_based = bool(char_based)
        self.n_ngrams = int(n_ngrams)
        self.vocab = list(vocab)
        self.alpha, self.beta = float(alpha), float(beta)
        self.n_lexicon_words, self.n_dropped_words = int(n_lexicon_words), int(n_dropped_words)

    def is_character_based(self) -> bool:
        return self._char_based

    def __repr__(self):
        return "ArpaLm(order=%d, n_ngrams=%d, %d bytes on %s, alpha=%g, beta=%g)" % (
            self.order, self.n_ngrams, self.image.numel(), self.image.device, self.alpha, self.beta)


def load_arpa(path, vocab, device="cuda", alpha: float = 1.0, beta: float = 1.0) -> ArpaLm:
    """Read a text ARPA LM for the class strings `vocab` (class c is vocab[c]; the blank is not part of it) and copy its image to
    `device`.  The mode is the file's: a character-based LM gives lasr_ctc_beam_decode_lm's image; a word-level LM, with a
    vocabulary that has exactly one " " label, the word image with its lexicon (ArpaLm.is_character_based() is False).  A missing
    file raises ArpaNotFoundError, one that cannot be read OSError; a KenLM binary model, or a word-level LM with a vocabulary
    that has no " " label or several, NotImplementedError; a malformed file, or an order outside 1..6, ValueError naming the line."""
    import numpy as np
    path = os.fspath(path)
    if not os.path.isfile(path):
        raise ArpaNotFoundError("no ARPA language model at %r" % (path,))
    lib = _lib.load()
    words = [str(w).encode("utf-8") for w in vocab]
    arr = (ctypes.c_char_p * max(len(words), 1))(*words)
    h = ctypes.c_void_p()
    spaces = [i for i, w in enumerate(words) if w == b" "]
    # with one space label the word-level build goes first, so that a (large) word-level file is read once; it declines a
    # character-based file, and anything else it rejects lasr_arpa_load rejects with its own message
    if len(spaces) == 1 and lib.lasr_arpa_load_words(os.fsencode(path), ctypes.cast(arr, ctypes.c_void_p), len(words), spaces[0],
                                                     ctypes.byref(h)) == 0:
        try:
            order, cb, n, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_size_t()
            call("lasr_arpa_info", h, ctypes.byref(order), ctypes.byref(cb), ctypes.byref(n), ctypes.byref(nb))
            n_lex, n_nodes, n_drop = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            call("lasr_arpa_lexicon_info", h, ctypes.byref(n_lex), ctypes.byref(n_nodes), ctypes.byref(n_drop))
            host = np.empty(int(nb.value), dtype=np.uint8)
            call("lasr_arpa_write_image", h, host.ctypes.data, int(nb.value))
        finally:
            lib.lasr_arpa_free(h)
        return ArpaLm(torch.from_numpy(host).to(device), order.value, False, n.value, vocab, alpha, beta, n_lex.value, n_drop.value)
    h = ctypes.c_void_p()
    rc = lib.lasr_arpa_load(os.fsencode(path), ctypes.cast(arr, ctypes.c_void_p), len(words), ctypes.byref(h))
    if rc != 0:
        msg = lib.lasr_last_error().decode(errors="replace")
        if rc == _E_UNSUPPORTED:
            raise NotImplementedError(msg)
        if rc == _E_IO:
            raise OSError(msg)
        raise ValueError(msg)
    try:
        order, cb, n, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_size_t()
        call("lasr_arpa_info", h, ctypes.byref(order), ctypes.byref(cb), ctypes.byref(n), ctypes.byref(nb))
        if not cb.value:
            raise NotImplementedError("%s is a word-level LM: only character-based LMs are supported (a word-level LM needs a "
                                      "space label and a dictionary FST): the vocabulary has %d \" \" labels, not one"
                                      % (path, len(spaces)))
        host = np.empty(int(nb.value), dtype=np.uint8)
        call("lasr_arpa_write_image", h, host.ctypes.data, int(nb.value))
    finally:
        lib.lasr_arpa_free(h)
    image = torch.from_numpy(host).to(device)
    return ArpaLm(image, order.value, True, n.value, vocab, alpha, beta)


def ctc_beam_decode_lm(logp: torch.Tensor, lens: Optional[torch.Tensor], blank: int, lm: ArpaLm, beam_width: int = 16,
                       cutoff_top_n: int = 40, cutoff_prob: float = 1.0, n_best: int = 1, alpha: Optional[float] = None,
                       beta: Optional[float] = None):
    """ctc_beam_decode fused with the n-gram LM `lm` (load_arpa; alpha / beta default to lm's).  Returns (tokens, n_tokens,
    scores, am_scores): scores are the fused log-scores the hypotheses are ranked by.  With a character-based LM am_scores are
    ctc_decoders' approx_ctc (fused - labels * beta - alpha * sentence LM score); with a word-level LM (lasr_ctc_beam_decode_wlm:
    only words of the LM's lexicon are decoded, each scored at the space after it or at the end of the utterance) they are the
    acoustic log-scores.  Shapes and ranges as ctc_beam_decode; the image must sit on logp's device and hold C - 1 labels."""
    who = "ctc_beam_decode_lm"
    # lm's type is checked after logp's and before any range, so a bad logp is left to _beam_args' own TypeError
    if not isinstance(lm, ArpaLm) and logp.dtype == torch.float32 and logp.dim() == 3:
        raise TypeError("lm must be an ArpaLm (ops.load_arpa)")
    B, T, Cc, cutoff_top_n = _beam_args(logp, lens, blank, beam_width, cutoff_top_n, cutoff_prob, n_best, who)
    alpha = lm.alpha if alpha is None else float(alpha)
    beta = lm.beta if beta is None else float(beta)
    if not (math.isfinite(alpha) and math.isfinite(beta)):
        raise ValueError("alpha %r / beta %r must be finite" % (alpha, beta))
    if len(lm.vocab) != Cc - 1:
        raise ValueError("the LM was loaded for %d labels; the log-probs have %d classes" % (len(lm.vocab), Cc))
    if lm.image.device != logp.device:
        raise ValueError("the LM image is on %s, the log-probs on %s" % (lm.image.device, logp.device))
    nb = int(_lib.load().lasr_ctc_beam_lm_workspace_bytes(B, T, Cc, beam_width, cutoff_top_n))
    if nb == 0:
        raise ValueError("ctc_beam_decode_lm: shape (%d, %d, %d) outside the kernel's range" % (B, T, Cc))
    tokens, n, scores = _beam_outputs(logp, n_best)
    am = torch.empty_like(scores)
    ws = _ws(nb, logp.device)
    entry = "lasr_ctc_beam_decode_lm" if lm.is_character_based() else "lasr_ctc_beam_decode_wlm"
    call(entry, _p(logp), _p(lens), B, T, Cc, int(blank), int(beam_width), int(cutoff_top_n), float(cutoff_prob),
         int(n_best), _p(lm.image), alpha, beta, _p(tokens), _p(n), _p(scores), _p(am), _p(ws), nb, _stream())
    return tokens, n, scores, am


HOTWORD_MAX_LEN = 32          # lasr_hotword_build's ranges (include/lasr.h)
HOTWORD_MAX_PHRASES = 65536


class HotwordBank:
    """A bank of phrases the beam search is biased towards (build_hotwords): the device image of its automaton, the number of
    phrases and trie nodes (the root included) and max_credit, the largest credit a node carries.  The host handle behind
    hotword_bonus is kept with the bank and freed with it."""

    def __init__(self, image: torch.Tensor, n_phrases: int, n_nodes: int, max_credit: float, n_classes: int, blank: int, handle=None):
        self.image = image
        self.n_phrases, self.n_nodes = int(n_phrases), int(n_nodes)
        self.max_credit = float(max_credit)
        self.n_classes, self.blank = int(n_classes), int(blank)
        self._handle = handle

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            try:
                _lib.load().lasr_hotword_free(h)
            except Exception:       # interpreter shutdown
                pass

    def __repr__(self):
        return "HotwordBank(n_phrases=%d, n_nodes=%d, max_credit=%g, %d bytes on %s)" % (
            self.n_phrases, self.n_nodes, self.max_credit, self.image.numel(), self.image.device)


def build_hotwords(phrases, weights=2.0, *, n_classes: int, blank: int, device="cuda") -> HotwordBank:
    """Build the biasing automaton of `phrases`, a list of label-id lists (1..32 ids in [0, n_classes), none the blank; an empty
    list is a valid bank that biases nothing), and copy its image to `device`.  `weights`: one float for all phrases or one per
    phrase, finite and > 0, in natural-log units per matched label.  The default 2.0 is a starting value: nobody has tuned it
    on a trained model.  A bad phrase or weight raises ValueError naming the phrase index."""
    import numpy as np
    phrases = [list(p) for p in phrases]
    n = len(phrases)
    if isinstance(weights, (int, float)):
        weights = [float(weights)] * n
    weights = [float(w) for w in weights]
    if len(weights) != n:
        raise ValueError("%d weights for %d phrases" % (len(weights), n))
    labels = np.asarray([c for p in phrases for c in p], dtype=np.int64)
    if labels.size and (labels.min() < -2 ** 31 or labels.max() >= 2 ** 31):
        raise ValueError("a label id outside the int32 range")
    labels = np.ascontiguousarray(labels.astype(np.int32))
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(p) for p in phrases], out=offsets[1:])
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32))
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.lasr_hotword_build(labels.ctypes.data if n else None, offsets.ctypes.data if n else None, w.ctypes.data if n else None,
                                n, int(n_classes), int(blank), ctypes.byref(h))
    if rc != 0:
        raise ValueError(lib.lasr_last_error().decode(errors="replace"))
    try:
        n_p, n_nodes, mc, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_float(), ctypes.c_size_t()
        call("lasr_hotword_info", h, ctypes.byref(n_p), ctypes.byref(n_nodes), ctypes.byref(mc), ctypes.byref(nb))
        host = np.empty(int(nb.value), dtype=np.uint8)
        call("lasr_hotword_write_image", h, host.ctypes.data, int(nb.value))
        image = torch.from_numpy(host).to(device)
    except Exception:
        lib.lasr_hotword_free(h)
        raise
    return HotwordBank(image, n_p.value, n_nodes.value, mc.value, n_classes, blank, h)


def hotword_bonus(bank: HotwordBank, ids):
    """The host walk of the label sequence `ids` over `bank`: (bonus, final, state) of that prefix (include/lasr.h: bonus is what
    the search adds while the prefix is live, final what it is worth at the end of the utterance, state the automaton node)."""
    import numpy as np
    if not isinstance(bank, HotwordBank) or not bank._handle:
        raise TypeError("bank must be a HotwordBank (ops.build_hotwords)")
    a = np.ascontiguousarray(np.asarray(list(ids), dtype=np.int32))
    b, f, st = ctypes.c_float(), ctypes.c_float(), ctypes.c_int32()
    lib = _lib.load()
    rc = lib.lasr_hotword_score(bank._handle, a.ctypes.data if a.size else None, int(a.size), ctypes.byref(b), ctypes.byref(f),
                                ctypes.byref(st))
    if rc != 0:
        raise ValueError(lib.lasr_last_error().decode(errors="replace"))
    return b.value, f.value, st.value


def ctc_beam_decode_biased(logp: torch.Tensor, lens: Optional[torch.Tensor], blank: int, bank: HotwordBank, beam_width: int = 16,
                           cutoff_top_n: int = 40, cutoff_prob: float = 1.0, n_best: int = 1, lm: Optional[ArpaLm] = None,
                           alpha: Optional[float] = None, beta: Optional[float] = None):
    """ctc_beam_decode (lm=None) or ctc_beam_decode_lm (a character-based `lm`) biased towards the phrases of `bank`
    (build_hotwords).  Returns (tokens, n_tokens, scores, am_scores, bias_scores): scores are what the hypotheses are ranked by,
    the acoustic (or LM-fused) score plus bias_scores, the phrase credit of each hypothesis; am_scores are the acoustic
    log-scores without an LM and ctc_decoders' approx_ctc with one.  Argument checks as ctc_beam_decode / ctc_beam_decode_lm;
    the bank must be built for logp's classes and blank and sit on its device.  A word-level LM raises NotImplementedError:
    its lexicon already confines the search to the LM's words."""
    who = "ctc_beam_decode_biased"
    if logp.dtype == torch.float32 and logp.dim() == 3:
        if not isinstance(bank, HotwordBank):
            raise TypeError("bank must be a HotwordBank (ops.build_hotwords)")
        if lm is not None and not isinstance(lm, ArpaLm):
            raise TypeError("lm must be an ArpaLm (ops.load_arpa) or None")
    B, T, Cc, cutoff_top_n = _beam_args(logp, lens, blank, beam_width, cutoff_top_n, cutoff_prob, n_best, who)
    if lm is not None and not lm.is_character_based():
        raise NotImplementedError("hotword biasing of the word-level LM search is not implemented: its lexicon confines the "
                                  "search to the LM's words")
    if bank.n_classes != Cc or bank.blank != blank:
        raise ValueError("the hotword bank was built for %d classes with blank %d; the log-probs have %d classes, blank %d"
                         % (bank.n_classes, bank.blank, Cc, blank))
    if bank.image.device != logp.device:
        raise ValueError("the hotword image is on %s, the log-probs on %s" % (bank.image.device, logp.device))
    nb = int(_lib.load().lasr_ctc_beam_workspace_bytes(B, T, Cc, beam_width, cutoff_top_n))
    if nb == 0:
        raise ValueError("%s: shape (%d, %d, %d) outside the kernel's range" % (who, B, T, Cc))
    if lm is not None:
        alpha = lm.alpha if alpha is None else float(alpha)
        beta = lm.beta if beta is None else float(beta)
        if not (math.isfinite(alpha) and math.isfinite(beta)):
            raise ValueError("alpha %r / beta %r must be finite" % (alpha, beta))
        if len(lm.vocab) != Cc - 1:
            raise ValueError("the LM was loaded for %d labels; the log-probs have %d classes" % (len(lm.vocab), Cc))
        if lm.image.device != logp.device:
            raise ValueError("the LM image is on %s, the log-probs on %s" % (lm.image.device, logp.device))
    tokens, n, scores = _beam_outputs(logp, n_best)
    am, bias = torch.empty_like(scores), torch.empty_like(scores)
    ws = _ws(nb, logp.device)
    if lm is None:
        call("lasr_ctc_beam_decode_bias", _p(logp), _p(lens), B, T, Cc, int(blank), int(beam_width), int(cutoff_top_n),
             float(cutoff_prob), int(n_best), _p(bank.image), _p(tokens), _p(n), _p(scores), _p(am), _p(bias), _p(ws), nb, _stream())
    else:
        call("lasr_ctc_beam_decode_lm_bias", _p(logp), _p(lens), B, T, Cc, int(blank), int(beam_width), int(cutoff_top_n),
             float(cutoff_prob), int(n_best), _p(lm.image), alpha, beta, _p(bank.image), _p(tokens), _p(n), _p(scores), _p(am),
             _p(bias), _p(ws), nb, _stream())
    return tokens, n, scores, am, bias


def _chunk_lens(lens, n_streams: int, t_chunk: int, device):
    """lens of one feed -> (device int32 tensor or None, per-stream upper bounds of the frames it adds).  A list or a host
    tensor is exact; a device tensor is not read back, so each stream is bounded by the chunk's length."""
    if lens is None:
        return None, [t_chunk] * n_streams
    if torch.is_tensor(lens) and lens.is_cuda:
        if lens.dtype != torch.int32 or lens.shape != (n_streams,):
            raise TypeError("lens must be (%d,) int32" % n_streams)
        return lens.contiguous(), [t_chunk] * n_streams
    host = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    if len(host) != n_streams:
        raise ValueError("%d lens for %d streams" % (len(host), n_streams))
    return torch.tensor(host, dtype=torch.int32).to(device), [min(max(v, 0), t_chunk) for v in host]


class CtcBeamStream:
    """The resumable CTC prefix beam search (lasr_ctc_beam_stream_*): `n_streams` sequences decoded chunk by chunk.  After every
    feed() the outputs are those of the one-shot decode (ctc_beam_decode / _lm / _biased) of the frames fed so far, bit for bit,
    however the frames were cut into chunks; the last feed's outputs are the final result.  lm: an ArpaLm (character or word),
    bank: a HotwordBank (not with a word LM); both, alpha and beta are fixed for the life of the object.  The object owns the
    state, the workspace and the output tensors; feed() returns views of the outputs, which the next feed overwrites.

    t_cap: the most frames a stream can take between two resets.  The host keeps an upper bound of the frames fed to each stream
    (exact when lens is None, a list or a host tensor; the chunk's length when lens is a device tensor) and feed() raises
    ValueError before launching when that bound would pass t_cap.  A feed replayed from a captured graph bypasses this
    bookkeeping: there the device's own clamp holds (frames past t_cap are counted in `dropped`, not searched)."""

    def __init__(self, n_streams: int, n_classes: int, blank: int, beam_width: int = 16, cutoff_top_n: int = 40,
                 cutoff_prob: float = 1.0, n_best: int = 1, t_cap: int = 3000, lm: Optional[ArpaLm] = None,
                 bank: Optional[HotwordBank] = None, alpha: Optional[float] = None, beta: Optional[float] = None, device="cuda"):
        if lm is not None and not isinstance(lm, ArpaLm):
            raise TypeError("lm must be an ArpaLm (ops.load_arpa) or None")
        if bank is not None and not isinstance(bank, HotwordBank):
            raise TypeError("bank must be a HotwordBank (ops.build_hotwords) or None")
        B, Cc, W = int(n_streams), int(n_classes), int(beam_width)
        topn = min(int(cutoff_top_n), Cc) if Cc >= 1 else int(cutoff_top_n)
        if B < 1 or int(t_cap) < 1:
            raise ValueError("n_streams %d / t_cap %d must be >= 1" % (B, int(t_cap)))
        if not 1 <= W <= CTC_BEAM_MAX_WIDTH:
            raise ValueError("beam_width %d outside 1..%d" % (W, CTC_BEAM_MAX_WIDTH))
        if not 1 <= topn <= CTC_BEAM_MAX_TOP_N:
            raise ValueError("cutoff_top_n %d outside 1..%d" % (topn, CTC_BEAM_MAX_TOP_N))
        if not 1 <= Cc <= CTC_BEAM_MAX_CLASSES:
            raise ValueError("%d classes: the beam decoder takes at most %d" % (Cc, CTC_BEAM_MAX_CLASSES))
        if not 1 <= n_best <= W:
            raise ValueError("n_best %d outside 1..beam_width (%d)" % (n_best, W))
        if not 0.0 < cutoff_prob <= 1.0:
            raise ValueError("cutoff_prob %r outside (0, 1]" % (cutoff_prob,))
        if not 0 <= blank < Cc:
            raise ValueError("blank %d outside [0, %d)" % (blank, Cc))
        if lm is not None and bank is not None and not lm.is_character_based():
            raise NotImplementedError("hotword biasing of the word-level LM search is not implemented: its lexicon confines the "
                                      "search to the LM's words")
        self.device = torch.device(device)
        if lm is not None:
            alpha = lm.alpha if alpha is None else float(alpha)
            beta = lm.beta if beta is None else float(beta)
            if not (math.isfinite(alpha) and math.isfinite(beta)):
                raise ValueError("alpha %r / beta %r must be finite" % (alpha, beta))
            if len(lm.vocab) != Cc - 1:
                raise ValueError("the LM was loaded for %d labels; the stream has %d classes" % (len(lm.vocab), Cc))
        if bank is not None and (bank.n_classes != Cc or bank.blank != blank):
            raise ValueError("the hotword bank was built for %d classes with blank %d; the stream has %d classes, blank %d"
                             % (bank.n_classes, bank.blank, Cc, blank))
        if lm is None:
            self.kind = _lib.BEAM_PLAIN if bank is None else _lib.BEAM_BIAS
        elif not lm.is_character_based():
            self.kind = _lib.BEAM_WLM
        else:
            self.kind = _lib.BEAM_LM if bank is None else _lib.BEAM_LM_BIAS
        self.n_streams, self.n_classes, self.blank, self.beam_width = B, Cc, int(blank), W
        self.cutoff_top_n, self.cutoff_prob, self.n_best, self.t_cap = topn, float(cutoff_prob), int(n_best), int(t_cap)
        self.lm, self.bank = lm, bank
        lib = _lib.load()
        self._state_bytes = int(lib.lasr_ctc_beam_stream_state_bytes(B, self.t_cap, W, self.kind))
        if self._state_bytes == 0:
            raise ValueError("CtcBeamStream: %d streams of t_cap %d at beam_width %d are outside the kernel's range" % (B, self.t_cap, W))
        dev = self.device
        self._state = torch.empty(self._state_bytes, dtype=torch.uint8, device=dev)
        self._ws, self._ws_bytes = None, 0
        self.tokens = torch.full((B, self.n_best, self.t_cap), -1, dtype=torch.int32, device=dev)
        self.n_tokens = torch.zeros(B, self.n_best, dtype=torch.int32, device=dev)
        self.scores = torch.zeros(B, self.n_best, dtype=torch.float32, device=dev)
        self.am_scores = torch.zeros_like(self.scores) if self.kind != _lib.BEAM_PLAIN else None
        self.bias_scores = torch.zeros_like(self.scores) if bank is not None else None
        self._n_frames = torch.zeros(B, dtype=torch.int32, device=dev)
        self._n_dropped = torch.zeros(B, dtype=torch.int32, device=dev)
        lm_image = None if lm is None else lm.image.to(dev)
        bias_image = None if bank is None else bank.image.to(dev)
        self._images = (lm_image, bias_image)          # kept alive: the scorer record holds their addresses
        self._scorer = _lib.BeamScorer(self.kind, _p(lm_image), float(alpha or 0.0), float(beta or 0.0), _p(bias_image),
                                       _p(self.am_scores), _p(self.bias_scores))
        self._fed = [0] * B
        self.reset()

    @property
    def frames(self) -> torch.Tensor:
        """(n_streams,) int32 on the device: the frames each stream has searched since its last reset"""
        return self._n_frames

    @property
    def dropped(self) -> torch.Tensor:
        """(n_streams,) int32 on the device: the frames fed beyond t_cap, counted and not searched"""
        return self._n_dropped

    def reset(self, rows=None) -> None:
        """Make the streams `rows` (a list of indices; None: all of them) the empty prefix again."""
        if rows is None:
            rows_t, n = None, 0
            self._fed = [0] * self.n_streams
        else:
            rows = [int(r) for r in rows]
            if any(not 0 <= r < self.n_streams for r in rows):
                raise ValueError("rows %r outside [0, %d)" % (rows, self.n_streams))
            if not rows:
                return
            rows_t, n = torch.tensor(rows, dtype=torch.int32).to(self.device), len(rows)
            for r in rows:
                self._fed[r] = 0
        call("lasr_ctc_beam_stream_reset", _p(self._state), self._state_bytes, self.n_streams, self.t_cap, self.beam_width, self.kind,
             _p(rows_t), n, _stream())
        if rows is None:
            self._n_frames.zero_()
            self._n_dropped.zero_()
        else:
            self._n_frames[rows_t.long()] = 0
            self._n_dropped[rows_t.long()] = 0

    def feed(self, logp: torch.Tensor, lens=None):
        """logp (n_streams, T_chunk, C) f32: the next frames of every stream; lens: how many of them per stream (None: all; 0:
        the stream idles).  Returns (tokens (B, n_best, t_cap), n_tokens, scores[, am_scores[, bias_scores]]) as the one-shot
        decode of this stream's kind returns them, for the frames fed so far."""
        if logp.dtype != torch.float32 or logp.dim() != 3:
            raise TypeError("CtcBeamStream.feed takes (B, T, C) float32 log-probs")
        B, T, Cc = logp.shape
        if B != self.n_streams or Cc != self.n_classes:
            raise ValueError("feed of shape %s to %d streams of %d classes" % (tuple(logp.shape), self.n_streams, self.n_classes))
        if logp.device != self._state.device:
            raise ValueError("the log-probs are on %s, the stream on %s" % (logp.device, self._state.device))
        lens_t, add = _chunk_lens(lens, B, T, self.device)
        for b in range(B):
            if self._fed[b] + add[b] > self.t_cap:
                raise ValueError("stream %d: %d frames fed + %d would pass t_cap %d; reset() it or build a larger stream"
                                 % (b, self._fed[b], add[b], self.t_cap))
        nb = int(_lib.load().lasr_ctc_beam_stream_workspace_bytes(B, T, Cc, self.beam_width, self.cutoff_top_n))
        if nb == 0:
            raise ValueError("CtcBeamStream.feed: chunk (%d, %d, %d) outside the kernel's range" % (B, T, Cc))
        if nb > self._ws_bytes:
            self._ws, self._ws_bytes = _ws(nb, self.device), nb
        call("lasr_ctc_beam_stream_feed", _p(logp), _p(lens_t), B, T, Cc, self.blank, self.beam_width, self.cutoff_top_n,
             self.cutoff_prob, self.n_best, ctypes.byref(self._scorer), _p(self._state), self._state_bytes, self.t_cap,
             _p(self.tokens), _p(self.n_tokens), _p(self.scores), _p(self._n_frames), _p(self._n_dropped), _p(self._ws),
             self._ws_bytes, _stream())
        for b in range(B):
            self._fed[b] += add[b]
        out = (self.tokens, self.n_tokens, self.scores)
        if self.am_scores is not None:
            out += (self.am_scores,)
        if self.bias_scores is not None:
            out += (self.bias_scores,)
        return out


class GreedyStream:
    """Greedy CTC decoding chunk by chunk, with CtcBeamStream's feed / reset: the last raw argmax id of each stream is carried
    over the chunk border, prepended to the next chunk's ids, and the token it yields again is dropped, so the tokens equal
    greedy_decode of the whole row however it was cut.  feed() takes the argmax ids, not log-probs."""

    def __init__(self, n_streams: int, blank: int, t_cap: int = 3000, device="cuda"):
        self.n_streams, self.blank, self.t_cap = int(n_streams), int(blank), int(t_cap)
        self.device = torch.device(device)
        B = self.n_streams
        self._tokens = torch.full((B, self.t_cap + 1), -1, dtype=torch.int32, device=self.device)   # last column: discarded writes
        self.n_tokens = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._carry = torch.full((B,), self.blank, dtype=torch.int32, device=self.device)
        self._n_frames = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._fed = [0] * B

    @property
    def tokens(self) -> torch.Tensor:
        return self._tokens[:, :self.t_cap]

    @property
    def frames(self) -> torch.Tensor:
        return self._n_frames

    def reset(self, rows=None) -> None:
        idx = slice(None) if rows is None else torch.tensor([int(r) for r in rows], dtype=torch.long).to(self.device)
        self._tokens[idx] = -1
        self.n_tokens[idx] = 0
        self._carry[idx] = self.blank
        self._n_frames[idx] = 0
        for b in (range(self.n_streams) if rows is None else rows):
            self._fed[int(b)] = 0

    def feed(self, ids: torch.Tensor, lens=None):
        """ids (n_streams, T_chunk) int32 argmax ids, lens as CtcBeamStream.feed.  Returns (tokens (B, t_cap), -1 past each
        hypothesis; n_tokens (B)) for the frames fed so far."""
        if ids.dtype != torch.int32 or ids.dim() != 2 or ids.shape[0] != self.n_streams:
            raise TypeError("GreedyStream.feed takes (%d, T) int32 ids" % self.n_streams)
        B, T = ids.shape
        lens_t, add = _chunk_lens(lens, B, T, self.device)
        for b in range(B):
            if self._fed[b] + add[b] > self.t_cap:
                raise ValueError("stream %d: %d frames fed + %d would pass t_cap %d" % (b, self._fed[b], add[b], self.t_cap))
        if lens_t is None:
            lens_t = torch.full((B,), T, dtype=torch.int32, device=self.device)
        lens_t = lens_t.clamp(0, T)
        ext = torch.cat([self._carry[:, None], ids], dim=1).contiguous()
        tok, n = greedy_decode(ext, (lens_t + 1).contiguous(), self.blank)
        drop = (self._carry != self.blank).to(torch.int64)                 # the carried label's token came out last feed
        col = torch.arange(T, device=self.device)[None, :]
        new = tok.gather(1, (col + drop[:, None]).clamp(max=T))
        n_new = n.to(torch.int64) - drop
        dst = self.n_tokens.to(torch.int64)[:, None] + col
        dst = torch.where((col < n_new[:, None]) & (dst < self.t_cap), dst, torch.full_like(dst, self.t_cap))
        self._tokens.scatter_(1, dst, new)
        self.n_tokens += n_new.to(torch.int32)
        last = ids.gather(1, (lens_t.to(torch.int64) - 1).clamp(min=0)[:, None])[:, 0]
        self._carry = torch.where(lens_t > 0, last, self._carry)
        self._n_frames += lens_t
        for b in range(B):
            self._fed[b] += add[b]
        return self.tokens, self.n_tokens


# ---------------------------------------------------------------------------------- optimiser
def novograd_workspace(n_tensors: int, n_elems: int, device) -> torch.Tensor:
    """a ZEROED workspace a caller keeps across novograd_step(ws=...) calls (every call leaves it zeroed)"""
    return torch.zeros(max(int(_lib.load().lasr_novograd_workspace_bytes(n_tensors, n_elems)), 256), dtype=torch.uint8, device=device)


def novograd_step(params, grads, exp_avg, exp_avg_sq, offsets, lr_dev, beta1=0.8, beta2=0.5, eps=1e-8, weight_decay=0.0,
                  grad_scale=1.0, ws: Optional[torch.Tensor] = None, ema: Optional[torch.Tensor] = None,
                  ema_state: Optional[torch.Tensor] = None, clip_state: Optional[torch.Tensor] = None):
    """ws: a workspace from novograd_workspace() kept by the caller - the step then issues no memset of its own.
    ema + ema_state (``ema_state()``): the weight EMA of the parameters, updated by the step's last kernel with the weight the
    device record yields ("Weight EMA"); both or neither.
    clip_state (``clip_state()``): gradient clipping and the non-finite guard, decided on the device inside the step's three launches
    ("Gradient clipping and the non-finite guard"); None: the step as it always was, kernel for kernel."""
    n_t = exp_avg_sq.numel()
    n = params.numel()
    nb = _lib.load().lasr_novograd_workspace_bytes(n_t, n)
    if clip_state is not None:
        if (ema is None) != (ema_state is None):
            raise ValueError("novograd_step: ema and ema_state come together")
        if ema is not None:
            _ema_check("novograd_step", ema, params)
        for who, st, need in (("ema_state", ema_state, ema_state_bytes), ("clip_state", clip_state, clip_state_bytes)):
            if st is not None and (st.dtype != torch.uint8 or st.numel() < need() or st.device != params.device):
                raise ValueError("novograd_step: %s has to come from ops.%s() on %s" % (who, who, params.device))
        keep = ws is not None
        if ws is None:
            ws = _ws(nb, params.device)
        call("lasr_novograd_step_clip", _p(params), _p(grads), _p(exp_avg), _p(exp_avg_sq), _p(offsets), n_t, n, _p(lr_dev), beta1,
             beta2, eps, weight_decay, grad_scale, _p(ws), ws.numel(), _stream(), _p(ema) if ema is not None else None,
             _p(ema_state) if ema_state is not None else None, int(keep), _p(clip_state))
        return
    if ema is not None or ema_state is not None:
        if ema is None or ema_state is None:
            raise ValueError("novograd_step: ema and ema_state come together")
        _ema_check("novograd_step", ema, params)
        if ema_state.dtype != torch.uint8 or ema_state.numel() < ema_state_bytes() or ema_state.device != params.device:
            raise ValueError("novograd_step: ema_state has to come from ops.ema_state() on %s" % (params.device,))
        keep = ws is not None
        if ws is None:
            ws = _ws(nb, params.device)
        call("lasr_novograd_step_ema", _p(params), _p(grads), _p(exp_avg), _p(exp_avg_sq), _p(offsets), n_t, n, _p(lr_dev), beta1,
             beta2, eps, weight_decay, grad_scale, _p(ws), ws.numel(), _stream(), _p(ema), _p(ema_state), int(keep))
        return
    if ws is not None:
        call("lasr_novograd_step_keep", _p(params), _p(grads), _p(exp_avg), _p(exp_avg_sq), _p(offsets), n_t, n, _p(lr_dev), beta1,
             beta2, eps, weight_decay, grad_scale, _p(ws), ws.numel(), _stream())
        return
    ws = _ws(nb, params.device)
    call("lasr_novograd_step", _p(params), _p(grads), _p(exp_avg), _p(exp_avg_sq), _p(offsets), n_t, n, _p(lr_dev), beta1,
         beta2, eps, weight_decay, grad_scale, _p(ws), nb, _stream())


# ---- gradient clipping and the non-finite guard ("Gradient clipping and the non-finite guard") ----
# lasr_clip_state: int64 steps; int64 skipped; int mode; float clip_val; int skip_nonfinite; float total_norm; float coef;
# int last_skipped (40 bytes)
_CLIP_STATE_FMT = "<qqififfi"
CLIP_MODES = {"off": 0, "norm": 1, "value": 2}


def clip_state_bytes() -> int:
    return int(_lib.load().lasr_clip_state_bytes())


def clip_state_host(algorithm: str = "off", clip_val: float = 0.0, skip_nonfinite: bool = False, steps: int = 0,
                    skipped: int = 0) -> bytes:
    """the host image of the device record (lasr_clip_state_init).  ValueError: an algorithm outside off / norm / value, a value
    that is negative or not finite, norm / value without a value > 0, a negative count"""
    if algorithm not in CLIP_MODES:
        raise ValueError("clip algorithm has to be one of %s, got %r" % (sorted(CLIP_MODES), algorithm))
    clip_val = float(clip_val)
    if not (math.isfinite(clip_val) and clip_val >= 0.0):
        raise ValueError("clip value has to be a finite number >= 0, got %r" % (clip_val,))
    if algorithm != "off" and not float(np.float32(clip_val)) > 0.0:
        raise ValueError("clip algorithm %r needs a value > 0, got %r" % (algorithm, clip_val))
    if int(steps) < 0 or int(skipped) < 0:
        raise ValueError("clip steps / skipped have to be >= 0, got %r / %r" % (steps, skipped))
    nb = clip_state_bytes()
    host = ctypes.create_string_buffer(nb)
    call("lasr_clip_state_init", host, nb, CLIP_MODES[algorithm], clip_val, int(bool(skip_nonfinite)), int(steps), int(skipped))
    return host.raw


def clip_state(algorithm: str = "off", clip_val: float = 0.0, skip_nonfinite: bool = False, steps: int = 0, skipped: int = 0,
               device="cuda") -> torch.Tensor:
    """The device record ``novograd_step(clip_state=...)`` reads and fills in: uint8 (lasr_clip_state_bytes()).  algorithm "off" with
    the guard off changes nothing in the step's arithmetic and still records the gradient norm.  ``clip_state_read`` reads it back."""
    return torch.frombuffer(bytearray(clip_state_host(algorithm, clip_val, skip_nonfinite, steps, skipped)), dtype=torch.uint8).to(device)


def clip_state_read(state) -> dict:
    """{"algorithm", "clip_val", "skip_nonfinite", "steps", "skipped", "total_norm", "coef", "last_skipped"} of a record (a tensor
    from ``clip_state`` - one device read - or host bytes).  steps counts the optimiser steps that went through the record, skipped
    those of them that were dropped as non-finite; the last three describe the LAST step.  total_norm is the global norm of the
    scaled gradient g^ = grad_scale * g as the norm kernel squared it: BEFORE the clip in norm mode, AFTER the clamp in value mode (the
    one quantity the kernels already hold); coef is what the update multiplied g^ by (1 outside norm mode)."""
    import struct
    raw = bytes(state.cpu().numpy().tobytes()) if torch.is_tensor(state) else bytes(state)
    steps, skipped, mode, c, guard, total_norm, coef, last = struct.unpack_from(_CLIP_STATE_FMT, raw)
    names = {v: k for k, v in CLIP_MODES.items()}
    return {"algorithm": names[mode], "clip_val": float(c), "skip_nonfinite": bool(guard), "steps": int(steps), "skipped": int(skipped),
            "total_norm": float(total_norm), "coef": float(coef), "last_skipped": bool(last)}


def clip_coef(total_norm, c) -> np.float32:
    """Host twin of the device coefficient of norm clipping, in numpy f32: min(1, f32(c) / (f32(total_norm) + f32(1e-6))) - one add,
    one division, the constants of ``torch.nn.utils.clip_grad_norm_``; a NaN stays a NaN."""
    with np.errstate(all="ignore"):
        q = np.float32(c) / (np.float32(total_norm) + np.float32(1e-6))
    return np.float32(1.0) if q > np.float32(1.0) else np.float32(q)


# ---- weight EMA ("Weight EMA") ----
_EMA_STATE_FMT = "<qfif"        # lasr_ema_state: int64 num_updates; float decay; int warmup; float w (padded to 24 bytes)


def ema_state_bytes() -> int:
    return int(_lib.load().lasr_ema_state_bytes())


def ema_state_host(decay: float, warmup: bool = True, num_updates: int = 0) -> bytes:
    """the host image of the device record (lasr_ema_state_init); ValueError for a decay outside [0, 1) or a negative count"""
    decay = float(decay)
    if not (math.isfinite(decay) and 0.0 <= decay < 1.0):
        raise ValueError("ema decay has to be in [0, 1), got %r" % (decay,))
    if int(num_updates) < 0:
        raise ValueError("ema num_updates has to be >= 0, got %r" % (num_updates,))
    nb = ema_state_bytes()
    host = ctypes.create_string_buffer(nb)
    call("lasr_ema_state_init", host, nb, decay, int(bool(warmup)), int(num_updates))
    return host.raw


def ema_state(decay: float, warmup: bool = True, num_updates: int = 0, device="cuda") -> torch.Tensor:
    """The device record the optimiser step advances: uint8 (lasr_ema_state_bytes()).  ``ema_state_read`` reads it back."""
    return torch.frombuffer(bytearray(ema_state_host(decay, warmup, num_updates)), dtype=torch.uint8).to(device)


def ema_state_read(state) -> dict:
    """{"num_updates", "decay", "warmup", "w"} of a record (a tensor from ``ema_state`` - one device read - or host bytes)"""
    import struct
    raw = bytes(state.cpu().numpy().tobytes()) if torch.is_tensor(state) else bytes(state)
    n, decay, warmup, w = struct.unpack_from(_EMA_STATE_FMT, raw)
    return {"num_updates": int(n), "decay": float(decay), "warmup": bool(warmup), "w": float(w)}


def ema_weight(decay: float, warmup: bool, t: int) -> np.float32:
    """Host twin of the device weight of EMA update number t (0-based), in numpy f32: d = min(decay, f32(1 + t) / f32(10 + t))
    with warm-up, else decay; w = 1 - d."""
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + int(t)) / np.float32(10 + int(t)))
    return np.float32(1.0) - np.float32(d)


def _ema_check(who: str, ema: torch.Tensor, params: torch.Tensor) -> None:
    for t in (ema, params):
        if t.dtype != torch.float32:
            raise TypeError("%s averages float32 buffers, got %s" % (who, t.dtype))
        if not t.is_cuda:
            raise _lib.LasrError("liblasr ops need GPU tensors (got a %s tensor); there is no CPU fallback" % t.device)
    if ema.dim() != 1 or params.dim() != 1 or ema.numel() != params.numel():
        raise ValueError("%s needs two flat buffers of one size, got %s and %s" % (who, tuple(ema.shape), tuple(params.shape)))
    if ema.device != params.device:
        raise ValueError("%s: buffers on %s and %s" % (who, ema.device, params.device))


def ema_update(ema: torch.Tensor, params: torch.Tensor, w) -> None:
    """``ema = ema + (params - ema) * w`` over two flat f32 GPU buffers of one size, in one launch and in the three roundings
    of the torch expression (bit-equal to it) - the update the fused optimiser step applies, with the weight from the host."""
    _ema_check("ema_update", ema, params)
    if ema.numel() == 0:
        return
    call("lasr_ema_update", _p(ema), _p(params), ema.numel(), float(w), _stream())


ACC_MAX_RANGES = 8          # LASR_ACC_MAX_RANGES


def grad_accumulate(acc: torch.Tensor, g: torch.Tensor, ranges=None) -> None:
    """``acc += g`` over two flat f32 GPU buffers of one size (bit-equal to torch's ``acc + g``), in one launch.  ranges:
    [(lo, hi), ...] element offsets, at most ACC_MAX_RANGES pieces that do not overlap (the pieces of an all-reduce bucket);
    None = the whole buffer."""
    for t in (acc, g):
        if t.dtype != torch.float32:
            raise TypeError("grad_accumulate adds float32 buffers, got %s" % t.dtype)
        if not t.is_cuda:
            raise _lib.LasrError("liblasr ops need GPU tensors (got a %s tensor); there is no CPU fallback" % t.device)
    if acc.dim() != 1 or g.dim() != 1 or acc.numel() != g.numel():
        raise ValueError("grad_accumulate needs two flat buffers of one size, got %s and %s" % (tuple(acc.shape), tuple(g.shape)))
    if acc.device != g.device:
        raise ValueError("grad_accumulate: buffers on %s and %s" % (acc.device, g.device))
    n = acc.numel()
    if n == 0:
        return
    if ranges is None:
        call("lasr_grad_accumulate", _p(acc), _p(g), n, _stream())
        return
    ranges = [(int(lo), int(hi)) for lo, hi in ranges]
    if len(ranges) > ACC_MAX_RANGES:
        raise ValueError("grad_accumulate takes at most %d ranges, got %d" % (ACC_MAX_RANGES, len(ranges)))
    if any(lo < 0 or hi < lo or hi > n for lo, hi in ranges):
        raise ValueError("grad_accumulate: a range outside [0, %d] or with lo > hi: %s" % (n, ranges))
    if not ranges:
        return
    lo = (ctypes.c_int64 * len(ranges))(*[r[0] for r in ranges])
    hi = (ctypes.c_int64 * len(ranges))(*[r[1] for r in ranges])
    call("lasr_grad_accumulate_ranges", _p(acc), _p(g), lo, hi, len(ranges), _stream())


def edit_distance_batch(tokens: torch.Tensor, n_tokens: torch.Tensor, targets: torch.Tensor, target_lens: torch.Tensor,
                        space_id: int = -1, totals: Optional[torch.Tensor] = None):
    """Levenshtein distance of every utterance on the device: tokens (B,T) i32 + n_tokens (B) i32 from greedy_decode,
    targets (B,S) i64 + target_lens (B) i32.  space_id < 0: per token (CER); >= 0: per word.  Returns (dist (B) i32,
    ref_units (B) i32); ``totals`` (2) i64, if given, is incremented by their sums (no host synchronisation)."""
    B = tokens.shape[0]
    dev = tokens.device
    dist = torch.empty(B, dtype=torch.int32, device=dev)
    units = torch.empty(B, dtype=torch.int32, device=dev)
    call("lasr_edit_distance_batch", _p(tokens), _p(n_tokens), tokens.shape[1], _p(targets), _p(target_lens), targets.shape[1], B,
         int(space_id), _p(dist), _p(units), _p(totals), _stream())
    return dist, units


EDIT_HIT, EDIT_SUB, EDIT_DEL, EDIT_INS, EDIT_PAD = 0, 1, 2, 3, 255      # LASR_EDIT_* (include/lasr.h)


class EditOps(NamedTuple):
    dist: torch.Tensor           # (B,) i32 Levenshtein distance, bit-equal to edit_distance_batch
    ref_units: torch.Tensor      # (B,) i32 reference units
    counts: torch.Tensor         # (B, 4) i32 hits, substitutions, deletions, insertions
    ops: torch.Tensor            # (B, T + S) u8 the script forwards (EDIT_HIT / SUB / DEL / INS), EDIT_PAD past n_ops
    n_ops: torch.Tensor          # (B,) i32 length of the script


def edit_ops_batch(tokens: torch.Tensor, n_tokens: torch.Tensor, targets: torch.Tensor, target_lens: torch.Tensor,
                   space_id: int = -1, totals: Optional[torch.Tensor] = None, confusion: Optional[torch.Tensor] = None) -> EditOps:
    """edit_distance_batch with the alignment behind the distance (include/lasr.h lasr_edit_align_batch: the canonical script -
    diagonal before deletion before insertion, walking back from the end): same inputs, same dist / ref_units.  ``totals`` (6)
    i64, if given, is incremented by the sums of dist, ref_units, hits, subs, dels, ins; ``confusion`` (n_classes + 1,
    n_classes + 1) i32, token units only, is incremented at [reference label][hypothesis label], index n_classes = none.
    One launch (two with totals), nothing synchronised."""
    if tokens.dim() != 2 or tokens.dtype != torch.int32 or targets.dim() != 2 or targets.dtype != torch.int64 \
            or targets.shape[0] != tokens.shape[0]:
        raise ValueError("edit_ops_batch takes tokens (B, T) int32 and targets (B, S) int64")
    B, T, S = tokens.shape[0], tokens.shape[1], targets.shape[1]
    for name, t in (("n_tokens", n_tokens), ("target_lens", target_lens)):
        if t.shape != (B,) or t.dtype != torch.int32:
            raise ValueError("edit_ops_batch: %s must be (B,) int32" % name)
    if totals is not None and (totals.dtype != torch.int64 or totals.numel() < 6):
        raise TypeError("totals must hold 6 int64 values")
    n_classes = 0
    if confusion is not None:
        if confusion.dim() != 2 or confusion.shape[0] != confusion.shape[1] or confusion.shape[0] < 2 or confusion.dtype != torch.int32:
            raise TypeError("confusion must be a square (n_classes + 1, n_classes + 1) int32 matrix")
        n_classes = confusion.shape[0] - 1
    dev = tokens.device
    out = EditOps(torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                  torch.empty(B, 4, dtype=torch.int32, device=dev), torch.empty(B, T + S, dtype=torch.uint8, device=dev),
                  torch.empty(B, dtype=torch.int32, device=dev))
    nb = int(_lib.load().lasr_edit_align_workspace_bytes(B, T, S))
    ws = _ws(nb, dev)
    call("lasr_edit_align_batch", _p(tokens), _p(n_tokens), T, _p(targets), _p(target_lens), S, B, int(space_id), _p(out.dist),
         _p(out.ref_units), _p(out.counts), _p(out.ops), T + S, _p(out.n_ops), _p(totals), _p(confusion), n_classes, _p(ws), nb, _stream())
    return out


def step_metrics(loss: torch.Tensor, dist: torch.Tensor, units: torch.Tensor, acc: torch.Tensor) -> None:
    """fold one step's loss and batch WER into the device accumulators acc (7 f64): see lasr_step_metrics"""
    if acc.dtype != torch.float64 or acc.numel() < 7:
        raise TypeError("acc must hold 7 float64 values")
    call("lasr_step_metrics", _p(loss), _p(dist), _p(units), dist.numel(), _p(acc), _stream())


# ---- sample-rate conversion (csrc/resample.hip; DESIGN.md "Resampling") ---------------------------------------------------
def resample_out_len(n_in: int, up: int, down: int) -> int:
    """ceil(n_in * up / down)"""
    n = _lib.load().lasr_resample_out_len(int(n_in), int(up), int(down))
    if n < 0:
        _lib.check(-1, "lasr_resample_out_len")
    return int(n)


class Resampler:
    """A bank of up to 8 rate conversions [(sr_in, sr_out), ...] built on the host and uploaded ONCE; a call converts a batch of
    rows on the device, each row by its own conversion (``conv_id``).  (1, 1)-like pairs (sr_in == sr_out) are plain copies."""

    def __init__(self, conversions, device="cuda", lpw: int = 6, rolloff: float = 0.99):
        conversions = [(int(a), int(b)) for a, b in conversions]
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.LasrError("Resampler runs on the GPU only (device=%r): there is no CPU path" % (device,))
        n = len(conversions)
        for a, b in conversions:                       # what does not fit the C ABI's int32 is refused here, with its rule
            if not (0 < a < 2 ** 31 and 0 < b < 2 ** 31):
                raise ValueError("Resampler: sample rates must be positive 31-bit integers, got %r" % ((a, b),))
        sr_in, sr_out = (ctypes.c_int32 * max(n, 1))(*[c[0] for c in conversions]), (ctypes.c_int32 * max(n, 1))(*[c[1] for c in conversions])
        lib = _lib.load()
        nbytes = lib.lasr_resample_bank_bytes(sr_in, sr_out, n, int(lpw), float(rolloff))
        if not nbytes:
            _lib.check(-1, "lasr_resample_bank_bytes")
        host = torch.empty(nbytes // 4, dtype=torch.int32)
        call("lasr_resample_bank_write", sr_in, sr_out, n, int(lpw), float(rolloff), host.data_ptr(), nbytes)
        self.conversions, self.lpw, self.rolloff = conversions, int(lpw), float(rolloff)
        self.factors = []                               # (up, down) per conversion, from the image's own header
        for i in range(n):
            up, down = int(host[16 + 8 * i]), int(host[17 + 8 * i])
            self.factors.append((up, down))
        self.bank = host.to(self.device)

    def out_len(self, n_in: int, conv: int = 0) -> int:
        up, down = self.factors[conv]
        return -((-int(n_in) * up) // down)

    def tile(self, conv: int = 0) -> int:
        """outputs per workgroup of conversion `conv` (where the kernel's tests put their row lengths)"""
        up, down = self.factors[conv]
        return int(_lib.load().lasr_resample_tile(up, down, self.lpw, self.rolloff))

    def __call__(self, wave: torch.Tensor, lens: Optional[torch.Tensor] = None, conv_id: Optional[torch.Tensor] = None, out_dtype=None,
                 out: Optional[torch.Tensor] = None, L_out: Optional[int] = None, out_lens: Optional[torch.Tensor] = None):
        """wave (B, L) f32 | int16 on the device (rows may be strided: stride(1) == 1) -> (out (B, L_out), out_lens (B) int32).
        lens (B) int32 valid samples per row (None = L); conv_id (B) int32 (None = conversion 0).  L_out defaults to the longest
        row any of the bank's conversions can produce from L samples; ``out`` (B, >= L_out) is written in place when given
        (columns past L_out are left alone), and so is ``out_lens`` (B) int32.  No host synchronisation."""
        if wave.dim() != 2 or wave.dtype not in (torch.float32, torch.int16) or not wave.is_cuda or (wave.shape[1] > 1 and wave.stride(1) != 1):
            raise _lib.LasrError("Resampler: wave must be a (B, L) f32 or int16 device tensor with contiguous rows")
        B, L = wave.shape
        in_pitch = wave.stride(0) if B > 1 else max(L, 1)
        if lens is None:
            lens = torch.full((B,), L, dtype=torch.int32, device=wave.device)
        if lens.dtype != torch.int32 or lens.numel() != B or not lens.is_cuda:
            raise _lib.LasrError("Resampler: lens must be a (B,) int32 device tensor")
        if conv_id is not None and (conv_id.dtype != torch.int32 or conv_id.numel() != B or not conv_id.is_cuda):
            raise _lib.LasrError("Resampler: conv_id must be a (B,) int32 device tensor")
        out_dtype = (out.dtype if out is not None else wave.dtype) if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.int16):
            raise _lib.LasrError("Resampler: out_dtype must be torch.float32 or torch.int16")
        if L_out is None:
            L_out = max(self.out_len(L, i) for i in range(len(self.factors))) if out is None else out.shape[1]
        if out is None:
            out = torch.empty(B, max(L_out, 1), dtype=out_dtype, device=wave.device)[:, :L_out]
        if out.dim() != 2 or out.shape[0] != B or out.shape[1] < L_out or out.dtype != out_dtype or not out.is_cuda or (out.shape[1] > 1 and out.stride(1) != 1):
            raise _lib.LasrError("Resampler: out must be a (B, >= L_out) device tensor of out_dtype with contiguous rows")
        out_pitch = out.stride(0) if B > 1 else max(out.shape[1], L_out)
        if out_lens is None:
            out_lens = torch.empty(B, dtype=torch.int32, device=wave.device)
        elif out_lens.dtype != torch.int32 or out_lens.numel() != B or not out_lens.is_cuda or not out_lens.is_contiguous():
            raise _lib.LasrError("Resampler: out_lens must be a contiguous (B,) int32 device tensor")
        code = lambda dt: _lib.WAVE_F32 if dt == torch.float32 else _lib.WAVE_PCM16  # noqa: E731
        call("lasr_resample", _p(self.bank), wave.data_ptr(), code(wave.dtype), in_pitch, _p(lens.contiguous()),
             _p(conv_id.contiguous()) if conv_id is not None else None, out.data_ptr(), code(out_dtype), out_pitch, L_out, _p(out_lens), B, _stream())
        return out[:, :L_out], out_lens


_RESAMPLERS: dict = {}


def resample(wave: torch.Tensor, sr_in: int, sr_out: int):
    """wave (B, L) or (L,) f32 | int16 on the device at sr_in -> (out, out_lens) at sr_out; the resampler of a (pair, device) is
    built once and kept."""
    w2 = wave.unsqueeze(0) if wave.dim() == 1 else wave
    dev = w2.device
    key = (int(sr_in), int(sr_out), dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    r = _RESAMPLERS.get(key)
    if r is None:
        r = _RESAMPLERS[key] = Resampler([(sr_in, sr_out)], w2.device)
    out, n = r(w2.contiguous())
    return (out[0] if wave.dim() == 1 else out), n


# ---- noise and reverberation (csrc/wave_aug.hip; DESIGN.md "Noise and reverberation") ---------------------------------------
def wave_augment_tile() -> int:
    """outputs per workgroup of the augmentation's FIR (where its tests put their row lengths)"""
    return int(_lib.load().lasr_wave_augment_tile())


def wave_augment_chunk() -> int:
    """taps the FIR stages per chunk (where its tests put their filter lengths)"""
    return int(_lib.load().lasr_wave_augment_chunk())


def _host_f32(a, what: str) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim != 1 or a.dtype not in (np.float32, np.int16):
        raise ValueError("%s must be a 1-D float32 or int16 host array" % what)
    return a.astype(np.float32) / 32768.0 if a.dtype == np.int16 else np.ascontiguousarray(a)


def rir_bank_image(rirs) -> torch.Tensor:
    """the RIR bank image (int32 words, host) of a list of 1-D f32 | int16 arrays: header table (taps K, delay d, offset per
    RIR; entry i at words 4 + 4 i) + taps.  LasrError naming the index for what the bank refuses (include/lasr.h)."""
    arrs = [_host_f32(r, "an RIR") for r in rirs]
    n = len(arrs)
    flat = np.ascontiguousarray(np.concatenate(arrs)) if n and sum(a.size for a in arrs) else np.zeros(1, dtype=np.float32)
    lens = (ctypes.c_int64 * max(n, 1))(*[a.size for a in arrs])
    lib = _lib.load()
    nbytes = lib.lasr_rir_bank_bytes(flat.ctypes.data, lens, n)
    if not nbytes:
        _lib.check(-1, "lasr_rir_bank_bytes")
    host = torch.empty(nbytes // 4, dtype=torch.int32)
    call("lasr_rir_bank_write", flat.ctypes.data, lens, n, host.data_ptr(), nbytes)
    return host


class WaveAugmenter:
    """Reverberation and additive noise on the device.  ``rirs`` / ``noises``: lists of 1-D f32 or int16 host arrays (either may be
    empty); both banks are built and uploaded ONCE, the noise held as PCM16 (f32 clips are rounded like every PCM16 store).  A call
    augments a batch of rows, each by its own parameter word (rir_id, noise_id, noise_start, snr_cdb), -1 = off."""

    def __init__(self, rirs, noises, device="cuda", noise_dtype=torch.int16):
        """noise_dtype=torch.float32 keeps f32 clips as they are (the kernel reads either); the default is the PCM16 bank"""
        self.device = torch.device(device)
        if noise_dtype not in (torch.float32, torch.int16):
            raise ValueError("WaveAugmenter: noise_dtype must be torch.float32 or torch.int16")
        self.noise_dtype = noise_dtype
        if self.device.type != "cuda":
            raise _lib.LasrError("WaveAugmenter runs on the GPU only (device=%r): there is no CPU path" % (device,))
        image = rir_bank_image(rirs)
        self.n_rir = int(image[1])
        self.rir_taps = [int(image[4 + 4 * i]) for i in range(self.n_rir)]
        self.rir_delay = [int(image[5 + 4 * i]) for i in range(self.n_rir)]
        self.rir_bank = image.to(self.device)
        clips, off, table = [], 0, []
        for i, c in enumerate(noises):
            a = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
            if a.ndim != 1 or a.dtype not in (np.float32, np.int16) or a.size < 1:
                raise ValueError("noise clip %d must be a non-empty 1-D float32 or int16 host array" % i)
            if noise_dtype == torch.float32:
                a = a.astype(np.float32) / 32768.0 if a.dtype == np.int16 else a
            elif a.dtype != np.int16:
                a = np.clip(np.rint(a.astype(np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)
            clips.append(a)
            table.append((off, a.size))
            off += a.size
        if off >= 2 ** 31:
            raise ValueError("the noise bank holds %d samples, 2^31 or more" % off)
        self.noise_lens = [t[1] for t in table]
        self.noise_total = off
        self.noise = torch.from_numpy(np.concatenate(clips) if clips else np.zeros(1, dtype=np.int16 if noise_dtype == torch.int16 else np.float32)).to(self.device)
        self.clips = torch.tensor(table if table else [(0, 0)], dtype=torch.int32).to(self.device)
        self.n_clips = len(table)
        self._ws = None

    def workspace(self, B: int, L: int) -> torch.Tensor:
        """the call's workspace, grown when a larger batch arrives (never inside a graph capture: size it with an eager call)"""
        need = int(_lib.load().lasr_wave_augment_workspace_bytes(int(B), int(L)))
        if need == 0 and B:
            _lib.check(-1, "lasr_wave_augment_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(int(need * 1.25) + 64, dtype=torch.uint8, device=self.device)
        return self._ws

    def fir_rows(self, B: int, L: int) -> torch.Tensor:
        """(B, L) f32 view of the workspace's y after a call with these sizes: the FIR's own output on the reverberated rows
        (whole tiles up to each row's length; other rows hold whatever was there) - what the kernel's tests measure"""
        pitch = -(-max(int(L), 1) // wave_augment_tile()) * wave_augment_tile()
        return self._ws[:B * pitch * 4].view(torch.float32).view(B, pitch)[:, :L]

    def __call__(self, wave: torch.Tensor, lens: Optional[torch.Tensor], params: torch.Tensor, out_dtype=None,
                 out: Optional[torch.Tensor] = None, out_lens: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None):
        """wave (B, L) f32 | int16 on the device (stride(1) == 1); lens (B) int32 length words (None = L); params (B, 4) int32 ->
        (out (B, L), out_lens (B) int32, stats (B, 3) f64 = E_x, E_y, E_n).  ``out`` may be ``wave`` itself.  lens and params may
        be HOST tensors: they are then checked (a row that is to be augmented must not carry LEN_LEAD) and uploaded; device
        tensors are taken as they are, without a host synchronisation.  workspace: a uint8 device block of at least
        lasr_wave_augment_workspace_bytes(B, L) bytes owned by the caller (None = this object's own)."""
        if wave.dim() != 2 or wave.dtype not in (torch.float32, torch.int16) or not wave.is_cuda or (wave.shape[1] > 1 and wave.stride(1) != 1):
            raise _lib.LasrError("WaveAugmenter: wave must be a (B, L) f32 or int16 device tensor with contiguous rows")
        B, L = wave.shape
        if params.dtype != torch.int32 or tuple(params.shape) != (B, 4):
            raise _lib.LasrError("WaveAugmenter: params must be a (B, 4) int32 tensor")
        if lens is None:
            lens = torch.full((B,), L, dtype=torch.int32, device=wave.device)
        if lens.dtype != torch.int32 or lens.numel() != B:
            raise _lib.LasrError("WaveAugmenter: lens must be a (B,) int32 tensor")
        if not lens.is_cuda and not params.is_cuda:
            flagged = (lens & _lib.LEN_LEAD).bool() & ((params[:, 0] >= 0) | (params[:, 1] >= 0))
            if bool(flagged.any()):
                raise ValueError("an augmented wave cannot carry a lead-in sample (row %d)" % int(flagged.nonzero()[0]))
        lens, params = lens.to(wave.device).contiguous(), params.to(wave.device).contiguous()
        out_dtype = (out.dtype if out is not None else wave.dtype) if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.int16):
            raise _lib.LasrError("WaveAugmenter: out_dtype must be torch.float32 or torch.int16")
        if out is None:
            out = torch.empty(B, max(L, 1), dtype=out_dtype, device=wave.device)[:, :L]
        if out.dim() != 2 or out.shape[0] != B or out.shape[1] < L or out.dtype != out_dtype or not out.is_cuda or (out.shape[1] > 1 and out.stride(1) != 1):
            raise _lib.LasrError("WaveAugmenter: out must be a (B, >= L) device tensor of out_dtype with contiguous rows")
        in_pitch = wave.stride(0) if B > 1 else max(L, 1)
        out_pitch = out.stride(0) if B > 1 else max(out.shape[1], L, 1)
        if out_lens is None:
            out_lens = torch.empty(B, dtype=torch.int32, device=wave.device)
        elif out_lens.dtype != torch.int32 or out_lens.numel() != B or not out_lens.is_cuda or not out_lens.is_contiguous():
            raise _lib.LasrError("WaveAugmenter: out_lens must be a contiguous (B,) int32 device tensor")
        if stats is None:
            stats = torch.empty(B, 3, dtype=torch.float64, device=wave.device)
        elif stats.dtype != torch.float64 or tuple(stats.shape) != (B, 3) or not stats.is_cuda or not stats.is_contiguous():
            raise _lib.LasrError("WaveAugmenter: stats must be a contiguous (B, 3) float64 device tensor")
        ws = self.workspace(B, L) if workspace is None else workspace
        code = lambda dt: _lib.WAVE_F32 if dt == torch.float32 else _lib.WAVE_PCM16  # noqa: E731
        call("lasr_wave_augment", _p(self.rir_bank), self.rir_bank.numel(), _p(self.noise), code(self.noise_dtype), _p(self.clips), self.n_clips,
             self.noise_total, wave.data_ptr(), code(wave.dtype), in_pitch, _p(lens), _p(params), out.data_ptr(), code(out_dtype),
             out_pitch, L, _p(out_lens), _p(stats), B, _p(ws), ws.numel(), _stream())
        return out[:, :L], out_lens, stats


# ---- long recordings (csrc/segment.hip; DESIGN.md "Inference: long recordings") ---------------------------------------------
class VadSegments(NamedTuple):
    segs: torch.Tensor           # (B, max_segments, 2) i32 (start, end) in samples; rows past n_segs are not written
    n_segs: torch.Tensor         # (B,) i32 the TRUE count: above max_segments only the first max_segments rows of segs are written
    floor: torch.Tensor          # (B,) i32 the noise floor level, before its clamps
    levels: Optional[torch.Tensor]   # (B, ceil(L / 160)) i16 frame levels 0..511 (the library's uint16), 0 past a row's frames, or None


def vad_sweep() -> int:
    """frames (and runs) one workgroup of the segmenter takes per sweep of its passes (where its tests put their row lengths)"""
    return int(_lib.load().lasr_vad_sweep())


def vad_params(on_db=12.0, off_db=6.0, floor_permille=100, min_level_db=-60.0, max_floor_db=-35.0, min_silence_s=0.3, min_speech_s=0.1,
               pad_s=0.1, max_segment_s=16.0) -> "_lib.VadParams":
    """the segmenter's integer parameters from dB and seconds (lasr_vad_params_from); LasrError for what its checks refuse"""
    p = _lib.VadParams()
    if not -2 ** 31 <= int(floor_permille) < 2 ** 31:
        raise ValueError("vad_params: floor_permille must lie in 1..1000")
    call("lasr_vad_params_from", float(on_db), float(off_db), int(floor_permille), float(min_level_db), float(max_floor_db),
         float(min_silence_s), float(min_speech_s), float(pad_s), float(max_segment_s), ctypes.byref(p))
    return p


def _wave_rows(wave: torch.Tensor, who: str):
    """a (B, L) f32 | int16 device tensor with contiguous rows -> (dtype code, row pitch)"""
    if wave.dim() != 2 or wave.dtype not in (torch.float32, torch.int16) or not wave.is_cuda or (wave.shape[1] > 1 and wave.stride(1) != 1):
        raise _lib.LasrError("%s: wave must be a (B, L) f32 or int16 device tensor with contiguous rows; there is no CPU path" % who)
    B, L = wave.shape
    pitch = wave.stride(0) if B > 1 else max(L, 1)
    if pitch < L:
        raise _lib.LasrError("%s: the rows of wave overlap" % who)
    return (_lib.WAVE_F32 if wave.dtype == torch.float32 else _lib.WAVE_PCM16), pitch


def vad_segments(wave: torch.Tensor, lens: Optional[torch.Tensor] = None, *, on_db=12.0, off_db=6.0, floor_permille=100,
                 min_level_db=-60.0, max_floor_db=-35.0, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1, max_segment_s=16.0,
                 max_segments=4096, return_levels=False) -> VadSegments:
    """Energy voice-activity segmentation of recordings at 16 kHz, one per row: wave (L,) or (B, L) f32 | int16 on the device (rows
    may be strided), lens (B) int32 samples per row (None = L).  A frame is 160 samples; its level is a quasi-log of its PCM16
    energy (0.376 dB a step).  Speech is what rises ``on_db`` above the noise floor (the ``floor_permille``-th permille of the
    row's levels, kept between ``min_level_db`` and ``max_floor_db`` dBFS) and everything around it down to ``off_db``; gaps shorter
    than ``min_silence_s`` are closed, runs shorter than ``min_speech_s`` dropped, the rest padded by ``pad_s`` and cut at its
    quietest frame wherever it is longer than ``max_segment_s``.  Integer arithmetic: exact, the same on every run.
    No host synchronisation; a 1-D wave gives results without the batch dimension."""
    one = wave.dim() == 1
    w2 = wave.unsqueeze(0) if one else wave
    code, pitch = _wave_rows(w2, "vad_segments")
    B, L = w2.shape
    dev = w2.device
    if lens is not None and (lens.dtype != torch.int32 or lens.numel() != B or not lens.is_cuda):
        raise _lib.LasrError("vad_segments: lens must be a (B,) int32 device tensor")
    max_segments = int(max_segments)
    if max_segments < 0:
        raise ValueError("vad_segments: max_segments must not be negative")
    p = vad_params(on_db, off_db, floor_permille, min_level_db, max_floor_db, min_silence_s, min_speech_s, pad_s, max_segment_s)
    F = -(-L // 160)
    segs = torch.empty(B, max_segments, 2, dtype=torch.int32, device=dev)
    n_segs = torch.empty(B, dtype=torch.int32, device=dev)
    floor = torch.empty(B, dtype=torch.int32, device=dev)
    levels = torch.empty(B, F, dtype=torch.int16, device=dev) if return_levels else None
    nb = int(_lib.load().lasr_vad_workspace_bytes(B, L))
    if nb == 0 and B:
        _lib.check(-1, "lasr_vad_workspace_bytes")
    ws = _ws(nb, dev)
    call("lasr_vad_segment", w2.data_ptr() if w2.numel() else None, code, pitch, _p(lens.contiguous()) if lens is not None else None, B, L,
         ctypes.byref(p), segs.data_ptr() if max_segments else None, max_segments, _p(n_segs), _p(floor),
         levels.data_ptr() if levels is not None and F else None, _p(ws), ws.numel(), _stream())
    if one:
        return VadSegments(segs[0], n_segs[0], floor[0], levels[0] if levels is not None else None)
    return VadSegments(segs, n_segs, floor, levels)


def gather_segments(wave: torch.Tensor, table, L_out: Optional[int] = None):
    """wave (L,) or (B, L) f32 | int16 on the device; table: n rows of (row, start, end) - a HOST int tensor, array or list (a
    device tensor is read back) -> (rows (n, L_out) of wave's dtype: samples [start, end) of the source row, then zeros;
    lens (n,) int32 = end - start).  L_out defaults to the longest segment; a segment longer than L_out is a LasrError
    (LASR_E_SHAPE), one outside its source row a ValueError.  One launch per 256 segments, no host synchronisation."""
    w2 = wave.unsqueeze(0) if wave.dim() == 1 else wave
    code, pitch = _wave_rows(w2, "gather_segments")
    B, L = w2.shape
    tab = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    tab = np.ascontiguousarray(tab.reshape(-1, 3)).astype(np.int64)
    n = tab.shape[0]
    bad = np.flatnonzero((tab[:, 0] < 0) | (tab[:, 0] >= B) | (tab[:, 1] < 0) | (tab[:, 2] < tab[:, 1]) | (tab[:, 2] > L))
    if bad.size:
        i = int(bad[0])
        raise ValueError("gather_segments: table[%d] = %s lies outside the (%d, %d) wave" % (i, tuple(int(v) for v in tab[i]), B, L))
    if L_out is None:
        L_out = int((tab[:, 2] - tab[:, 1]).max()) if n else 0
    L_out = int(L_out)
    if L_out < 0:
        raise ValueError("gather_segments: L_out must not be negative")
    out = torch.empty(n, L_out, dtype=w2.dtype, device=w2.device)
    lens = torch.empty(n, dtype=torch.int32, device=w2.device)
    tab32 = np.ascontiguousarray(tab.astype(np.int32))
    if n:
        call("lasr_segment_gather", w2.data_ptr(), code, pitch, tab32.ctypes.data, n, out.data_ptr() if L_out else None, L_out, _p(lens),
             _stream())
    return out, lens
