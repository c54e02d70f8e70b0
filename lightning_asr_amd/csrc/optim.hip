// Multi-tensor NovoGrad over flat f32 buffers: two launches per step for any number of tensors.
// Replaces scheduler/novograd.py:75-145 (betas=(0.8,0.5), eps=1e-8, weight_decay; no amsgrad,
// grad_averaging or luc: train.py:46), which issues ~10 tiny kernels per parameter tensor.
#include "common.h"
#include <cfloat>

namespace lasr {

// Stage 1: every workgroup owns a 16K-element slice of the flat gradient, walks the tensor segments
// that intersect it and adds each segment's sum of squares to norm2[tensor] (f64 atomics: a handful
// per workgroup; f64 keeps the result independent of arrival order to well below f32 resolution).
static constexpr int kNormChunk = 16384;

// Gradient clipping and the non-finite guard ("Gradient clipping and the non-finite guard"): one device record, like
// EmaState.  The run's configuration (mode, clip_val, skip_nonfinite) is written once by the host; the rest is written by thread 0
// of the moment kernel of every step, with ordinary stores, and read by the update kernel of the SAME step (coef, last_skipped).
enum { kClipOff = 0, kClipNorm = 1, kClipValue = 2 };
struct ClipState {
  int64_t steps;        // optimiser steps that passed through the record (skipped ones included)
  int64_t skipped;      // of them, skipped as non-finite
  int mode;
  float clip_val;
  int skip_nonfinite;
  float total_norm;     // last step: (float)sqrt(sum over all tensors of the squares the norm kernel took) - pre-clip by norm, post-clamp by value
  float coef;           // last step: what the update multiplied the gradient by (1 outside norm mode)
  int last_skipped;
};

// the bound of the value clamp: c in value mode, +Inf otherwise (clamp_keep_nan(v, Inf) == v for every v, bit for bit)
__device__ __forceinline__ float clip_value_bound(const ClipState* st) { return st->mode == kClipValue ? st->clip_val : INFINITY; }

// torch.clamp(v, -c, c): +-Inf becomes +-c and NaN stays NaN (both comparisons are false for it; fminf / fmaxf would return c)
__device__ __forceinline__ float clamp_keep_nan(float v, float c) { return v < -c ? -c : (v > c ? c : v); }

// kClip: every scaled gradient passes the value clamp before it is squared (the bound comes from the record)
template <bool kClip>
__device__ __forceinline__ void novograd_norm_body(const float* __restrict__ grads, const int64_t* __restrict__ offsets, int n_tensors,
                                                   int64_t n, double* __restrict__ norm2, float grad_scale,
                                                   const ClipState* __restrict__ clip_st) {
  __shared__ double s_red[4];
  float cl = 0.f;
  if constexpr (kClip) cl = clip_value_bound(clip_st);
  const int64_t beg = (int64_t)blockIdx.x * kNormChunk;
  const int64_t end = beg + kNormChunk < n ? beg + kNormChunk : n;
  int lo = 0, hi = n_tensors;  // offsets[lo] <= beg < offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= beg) lo = mid; else hi = mid;
  }
  int64_t seg = beg;
  for (int t = lo; t < n_tensors && seg < end; ++t) {
    const int64_t tend = offsets[t + 1] < end ? offsets[t + 1] : end;
    double acc = 0.0;
    int64_t e0 = seg;
    if ((seg & 3) == 0) {   // 16-byte groups of the segment (every tensor of the model starts on one), scalar tail
      const int64_t nv = (tend - seg) >> 2;
      // four 16-byte loads in flight per thread (clamped address, masked value): a 64 KB slice is 4 rounds instead of 16 dependent trips
      // (round 3: 13.6 -> 10.1 us.  Round 5 tried sixteen in flight - one round per slice: 10.8 -> 18.2 us, the short tensors' slices
      // then issue sixteen clamped duplicate loads each)
      constexpr int kInFlight = 4;
      for (int64_t q0 = threadIdx.x; q0 < nv; q0 += kInFlight * 256) {
        float4 g4[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) g4[u] = *reinterpret_cast<const float4*>(grads + seg + 4 * min(q0 + 256 * u, nv - 1));
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
          const float mk = q0 + 256 * u < nv ? grad_scale : 0.f;
          float a = g4[u].x * mk, b = g4[u].y * mk, c = g4[u].z * mk, d = g4[u].w * mk;
          if constexpr (kClip) {
            // a masked duplicate of an Inf is 0 * Inf = NaN: as ever where the live lane's Inf makes the sum non-finite anyway (off and
            // norm mode: cl = Inf, nothing changes), but in value mode the live lane's Inf is clamped to a finite c - the masked lanes
            // then have to add exactly nothing
            const bool live = q0 + 256 * u < nv || cl == INFINITY;
            a = live ? clamp_keep_nan(a, cl) : 0.f, b = live ? clamp_keep_nan(b, cl) : 0.f;
            c = live ? clamp_keep_nan(c, cl) : 0.f, d = live ? clamp_keep_nan(d, cl) : 0.f;
          }
          acc += ((double)a * (double)a + (double)b * (double)b) + ((double)c * (double)c + (double)d * (double)d);
        }
      }
      e0 = seg + 4 * nv;
    }
    for (int64_t e = e0 + threadIdx.x; e < tend; e += 256) {
      float g = grads[e] * grad_scale;
      if constexpr (kClip) g = clamp_keep_nan(g, cl);
      acc += (double)g * (double)g;
    }
    acc = wave_sum_d(acc);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && tend > seg) atomicAdd(&norm2[t], (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
    seg = tend;
  }
}

// (the clip variants are kernels of their own names: a step without a clip record launches the kernels it always launched, by name)
__global__ __launch_bounds__(256) void novograd_norm_kernel(const float* __restrict__ grads, const int64_t* __restrict__ offsets,
                                                            int n_tensors, int64_t n, double* __restrict__ norm2, float grad_scale) {
  novograd_norm_body<false>(grads, offsets, n_tensors, n, norm2, grad_scale, nullptr);
}
__global__ __launch_bounds__(256) void novograd_norm_kernel_clip(const float* __restrict__ grads, const int64_t* __restrict__ offsets,
                                                                 int n_tensors, int64_t n, double* __restrict__ norm2, float grad_scale,
                                                                 const ClipState* __restrict__ clip_st) {
  novograd_norm_body<true>(grads, offsets, n_tensors, n, norm2, grad_scale, clip_st);
}

// Weight EMA ("Weight EMA"): the record lives on the device, so a captured graph replays the decay warm-up like the LR
// schedule.  num_updates = EMA updates done so far; w = 1 - d is what the update kernel of the SAME step reads.
struct EmaState {
  int64_t num_updates;
  float decay;
  int warmup;
  float w;
};

// the weight of update number t (0-based) - one correctly rounded f32 division, one f32 subtraction; ops.ema_weight is its host twin
__device__ __forceinline__ float ema_weight(float decay, int warmup, int64_t t) {
  float d = decay;
  if (warmup) d = fminf(decay, __fdiv_rn((float)(1 + t), (float)(10 + t)));
  return __fsub_rn(1.0f, d);
}

// e <- e + (p - e) w in three f32 operations of one rounding each (no FMA contraction): bit-equal to torch's `e + (p - e) * w`
// (contraction is switched off for the block: the compiler's default would fuse the product and the sum into one FMA, and the
// __f*_rn intrinsics are plain operators to it)
__device__ __forceinline__ float ema_lerp(float e, float p, float w) {
#pragma clang fp contract(off)
  const float diff = p - e;
  const float prod = w * diff;
  return e + prod;
}

// Stage 2: v_i <- first ? ||g||^2 : b2 v + (1-b2)||g||^2 ; denom_i = sqrt(v_i)+eps ; norm2 re-zeroed
// kEma: thread 0 also advances the EMA record - it runs between the norm and the update, so the update kernel reads this step's w
template <bool kEma>
__global__ __launch_bounds__(256) void novograd_moment_kernel(double* __restrict__ norm2, float* __restrict__ exp_avg_sq,
                                                              float* __restrict__ denom, int n_tensors, float beta2, float eps,
                                                              EmaState* __restrict__ ema_st) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (kEma) {
    if (i == 0) {
      const int64_t t = ema_st->num_updates;
      ema_st->w = ema_weight(ema_st->decay, ema_st->warmup, t);
      ema_st->num_updates = t + 1;
    }
  }
  if (i >= n_tensors) return;
  const float norm = (float)norm2[i];
  norm2[i] = 0.0;
  float v = exp_avg_sq[i];
  v = (v == 0.f) ? norm : beta2 * v + (1.f - beta2) * norm;  // "if exp_avg_sq == 0: copy" novograd.py:115
  exp_avg_sq[i] = v;
  denom[i] = sqrtf(v) + eps;
}

// the clip coefficient of torch.nn.utils.clip_grad_norm_: min(1, c / (N + 1e-6)) in one correctly rounded f32 add and one division; a
// NaN stays a NaN (`q > 1` is false for it).  ops.clip_coef is its host twin
__device__ __forceinline__ float clip_coef(float total_norm, float c) {
  const float q = __fdiv_rn(c, __fadd_rn(total_norm, 1e-6f));
  return q > 1.0f ? 1.0f : q;
}

// Stage 2 with a clip record: the step's one decision is taken here, between the norm and the update.  The global norm needs every
// norm2[t] before any of them is zeroed, so the kernel is ONE workgroup: it stages the sums of squares through LDS, thread 0 adds them
// in f64 in tensor index order, decides (coef, skip), writes the record and - unless the step is skipped - advances the EMA record;
// after the barrier every thread strides over the tensors: the moment update (unless skipped) and the re-zeroing (always).
static constexpr int kMomentStage = 2048;
template <bool kEma>
__global__ __launch_bounds__(256) void novograd_moment_kernel_clip(double* __restrict__ norm2, float* __restrict__ exp_avg_sq,
                                                                   float* __restrict__ denom, int n_tensors, float beta2, float eps,
                                                                   EmaState* __restrict__ ema_st, ClipState* __restrict__ clip_st) {
  __shared__ double s_n2[kMomentStage];
  __shared__ float s_coef;
  __shared__ int s_skip;
  double total2 = 0.0;       // (thread 0's)
  for (int base = 0; base < n_tensors; base += kMomentStage) {
    const int cnt = n_tensors - base < kMomentStage ? n_tensors - base : kMomentStage;
    for (int i = threadIdx.x; i < cnt; i += 256) s_n2[i] = norm2[base + i];
    __syncthreads();
    if (threadIdx.x == 0) {
      int i = 0;
      for (; i + 8 <= cnt; i += 8) {     // eight LDS reads in flight ahead of the eight dependent adds
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = s_n2[i + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) total2 += v[u];
      }
      for (; i < cnt; ++i) total2 += s_n2[i];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int mode = clip_st->mode;
    const float total_norm = (float)sqrt(total2);
    const float coef = mode == kClipNorm ? clip_coef(total_norm, clip_st->clip_val) : 1.0f;
    const int skip = clip_st->skip_nonfinite != 0 && !isfinite(total2);
    clip_st->steps = clip_st->steps + 1;
    clip_st->skipped = clip_st->skipped + skip;
    clip_st->total_norm = total_norm;
    clip_st->coef = coef;
    clip_st->last_skipped = skip;
    if constexpr (kEma) {
      if (!skip) {
        const int64_t t = ema_st->num_updates;
        ema_st->w = ema_weight(ema_st->decay, ema_st->warmup, t);
        ema_st->num_updates = t + 1;
      }
    }
    s_coef = coef;
    s_skip = skip;
  }
  __syncthreads();
  const bool skip = s_skip != 0;
  const double coef2 = (double)s_coef * (double)s_coef;     // (coef == 1: 1.0 * n2 is n2 - every bit of the step is the un-clipped step's)
  for (int i = threadIdx.x; i < n_tensors; i += 256) {
    const double n2 = norm2[i];
    norm2[i] = 0.0;
    if (skip) continue;
    const float norm = (float)(coef2 * n2);
    float v = exp_avg_sq[i];
    v = (v == 0.f) ? norm : beta2 * v + (1.f - beta2) * norm;
    exp_avg_sq[i] = v;
    denom[i] = sqrtf(v) + eps;
  }
}

// kEma: the new parameters are also folded into the average `ema` while they are still in registers (one more 16-byte load and
// store per group, no launch); the kEma = false instantiation is the kernel as it always was
// kClip: the skip flag, the coefficient and the clamp bound are read once per thread next to lr; a skipped step returns before any store,
// otherwise the scaled gradient is clamped (value mode) and multiplied by coef (1 outside norm mode) in registers
template <bool kEma, bool kClip>
__device__ __forceinline__ void novograd_update_body(float* __restrict__ params, const float* __restrict__ grads,
                                                     float* __restrict__ exp_avg, const int64_t* __restrict__ offsets,
                                                     int n_tensors, const float* __restrict__ denom,
                                                     const float* __restrict__ lr_ptr, float beta1, float wd,
                                                     float grad_scale, int64_t n, float* __restrict__ ema,
                                                     const EmaState* __restrict__ ema_st, const ClipState* __restrict__ clip_st,
                                                     const int64_t first_grp, const int64_t grid_grps) {
  // The tensor of an element is found by bisection over the offset table: the table lives in LDS (a search from
  // global memory is seven dependent loads per element) and one search serves four consecutive elements, which
  // move as 16-byte vectors whenever the group lies inside one tensor (always, for this model's shapes).
  extern __shared__ int64_t s_off[];   // [n_tensors + 1]
  for (int i = threadIdx.x; i <= n_tensors; i += 256) s_off[i] = offsets[i];
  __syncthreads();
  const float lr = *lr_ptr;
  float w = 0.f;
  if constexpr (kEma) w = ema_st->w;
  float coef = 1.f, cl = 0.f;
  if constexpr (kClip) {
    if (clip_st->last_skipped) return;
    coef = clip_st->coef;
    cl = clip_value_bound(clip_st);
  }
  const int64_t ngrp = (n + 3) >> 2;
  for (int64_t q = first_grp; q < ngrp; q += grid_grps) {
    const int64_t e = 4 * q;
    int lo = 0, hi = n_tensors;  // s_off[lo] <= e < s_off[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_off[mid] <= e) lo = mid; else hi = mid;
    }
    if (e + 4 <= n && s_off[lo + 1] >= e + 4) {
      const float dn = denom[lo];
      const float4 p = *reinterpret_cast<const float4*>(params + e);
      const float4 g = *reinterpret_cast<const float4*>(grads + e);
      const float4 m0 = *reinterpret_cast<const float4*>(exp_avg + e);
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (kEma) a = *reinterpret_cast<const float4*>(ema + e);
      float pv[4] = {p.x, p.y, p.z, p.w}, gv[4] = {g.x, g.y, g.z, g.w}, mv[4] = {m0.x, m0.y, m0.z, m0.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float gs = gv[i] * grad_scale;
        if constexpr (kClip) gs = clamp_keep_nan(gs, cl) * coef;
        float gi = gs / dn;
        if (wd != 0.f) gi = gi + wd * pv[i];
        mv[i] = mv[i] * beta1 + gi;
        pv[i] = pv[i] - lr * mv[i];
      }
      *reinterpret_cast<float4*>(exp_avg + e) = make_float4(mv[0], mv[1], mv[2], mv[3]);
      *reinterpret_cast<float4*>(params + e) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      if constexpr (kEma)
        *reinterpret_cast<float4*>(ema + e) =
            make_float4(ema_lerp(a.x, pv[0], w), ema_lerp(a.y, pv[1], w), ema_lerp(a.z, pv[2], w), ema_lerp(a.w, pv[3], w));
    } else {
      for (int64_t ee = e; ee < e + 4 && ee < n; ++ee) {
        while (lo + 1 < n_tensors && s_off[lo + 1] <= ee) ++lo;
        const float pe = params[ee];
        float gs = grads[ee] * grad_scale;
        if constexpr (kClip) gs = clamp_keep_nan(gs, cl) * coef;
        float gi = gs / denom[lo];
        if (wd != 0.f) gi = gi + wd * pe;
        const float m = exp_avg[ee] * beta1 + gi;
        exp_avg[ee] = m;
        const float pn = pe - lr * m;
        params[ee] = pn;
        if constexpr (kEma) ema[ee] = ema_lerp(ema[ee], pn, w);
      }
    }
  }
}

template <bool kEma>
__global__ __launch_bounds__(256) void novograd_update_kernel(float* __restrict__ params, const float* __restrict__ grads,
                                                              float* __restrict__ exp_avg, const int64_t* __restrict__ offsets,
                                                              int n_tensors, const float* __restrict__ denom,
                                                              const float* __restrict__ lr_ptr, float beta1, float wd,
                                                              float grad_scale, int64_t n, float* __restrict__ ema,
                                                              const EmaState* __restrict__ ema_st) {
  novograd_update_body<kEma, false>(params, grads, exp_avg, offsets, n_tensors, denom, lr_ptr, beta1, wd, grad_scale, n, ema, ema_st, nullptr,
                                   blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}
template <bool kEma>
__global__ __launch_bounds__(256) void novograd_update_kernel_clip(float* __restrict__ params, const float* __restrict__ grads,
                                                                   float* __restrict__ exp_avg, const int64_t* __restrict__ offsets,
                                                                   int n_tensors, const float* __restrict__ denom,
                                                                   const float* __restrict__ lr_ptr, float beta1, float wd,
                                                                   float grad_scale, int64_t n, float* __restrict__ ema,
                                                                   const EmaState* __restrict__ ema_st,
                                                                   const ClipState* __restrict__ clip_st) {
  novograd_update_body<kEma, true>(params, grads, exp_avg, offsets, n_tensors, denom, lr_ptr, beta1, wd, grad_scale, n, ema, ema_st, clip_st,
                                  blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// Gradient accumulation: acc[i] = acc[i] + g[i] over up to LASR_ACC_MAX_RANGES [lo, hi) pieces of two flat f32 buffers in ONE
// launch (the pieces of an all-reduce bucket).  The host cuts every piece into a 4-byte head up to the first 16-byte boundary,
// a body of 16-byte groups and a 4-byte tail, and numbers the "units" of all pieces consecutively: the body's groups first, then
// the head's and the tail's single elements.  A piece whose two bases are not congruent mod 16 bytes is all single elements.
// The table travels by value in the kernel arguments; the grid strides over the units.  One plain add per element, one rounding.
struct AccRanges {
  int64_t body[LASR_ACC_MAX_RANGES];   // element offset of the first 16-byte group
  int64_t lo[LASR_ACC_MAX_RANGES];     // element offset of the piece
  int64_t hi[LASR_ACC_MAX_RANGES];
  int64_t nvec[LASR_ACC_MAX_RANGES];   // 16-byte groups
  int64_t first[LASR_ACC_MAX_RANGES + 1];   // first unit of the piece; [n] = all units
  int n;
};

__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, AccRanges r) {
  const int64_t total = r.first[r.n];
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    int k = 0;
    while (k + 1 < r.n && r.first[k + 1] <= u) ++k;
    const int64_t q = u - r.first[k];
    if (q < r.nvec[k]) {
      const int64_t e = r.body[k] + 4 * q;
      float4 a = *reinterpret_cast<const float4*>(acc + e);
      const float4 b = *reinterpret_cast<const float4*>(g + e);
      a.x = __fadd_rn(a.x, b.x);
      a.y = __fadd_rn(a.y, b.y);
      a.z = __fadd_rn(a.z, b.z);
      a.w = __fadd_rn(a.w, b.w);
      *reinterpret_cast<float4*>(acc + e) = a;
    } else {
      const int64_t s = q - r.nvec[k];                   // single elements: the head, then the tail
      const int64_t head = r.body[k] - r.lo[k];
      const int64_t e = s < head ? r.lo[k] + s : r.body[k] + 4 * r.nvec[k] + (s - head);
      if (e < r.hi[k]) acc[e] = __fadd_rn(acc[e], g[e]);
    }
  }
}

// Weight EMA outside a step: e[i] = e[i] + (p[i] - e[i]) w with w from the host, the expression of the fused update.  Like the
// accumulate kernel: a 4-byte head up to the first 16-byte boundary, 16-byte groups, a 4-byte tail; two bases that are not
// congruent mod 16 bytes move by single elements (nvec = 0, head = n).  Units: the groups first, then the head's and the tail's.
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n, int64_t head,
                                                         int64_t nvec, float w) {
  const int64_t total = nvec + (n - 4 * nvec);
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    if (u < nvec) {
      const int64_t e = head + 4 * u;
      float4 a = *reinterpret_cast<const float4*>(ema + e);
      const float4 b = *reinterpret_cast<const float4*>(p + e);
      a.x = ema_lerp(a.x, b.x, w);
      a.y = ema_lerp(a.y, b.y, w);
      a.z = ema_lerp(a.z, b.z, w);
      a.w = ema_lerp(a.w, b.w, w);
      *reinterpret_cast<float4*>(ema + e) = a;
    } else {
      const int64_t s = u - nvec;
      const int64_t e = s < head ? s : head + 4 * nvec + (s - head);
      if (e < n) ema[e] = ema_lerp(ema[e], p[e], w);
    }
  }
}

// f32 -> bf16 copy of a flat buffer (weights for the bf16 MFMA kernels)
__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t n) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    out[e] = f32_to_bf16(in[e]);
}

// out[r][c] = bf16(in[r][c]) for c < cols, 0 for cols <= c < ld_out: a bf16 copy whose rows start on 16-byte
// boundaries (ld_out % 8 == 0) so that GEMMs over a narrow matrix (the 28-class logit gradient) take the
// aligned operand path.
__global__ __launch_bounds__(256) void cast_pad_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t rows,
                                                            int64_t cols, int64_t ld_out) {
  const int64_t total = rows * ld_out;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ld_out, c = i - r * ld_out;
    out[i] = c < cols ? f32_to_bf16(in[r * cols + c]) : (bf16_t)0;
  }
}

}  // namespace lasr

using namespace lasr;

extern "C" size_t lasr_novograd_workspace_bytes(int64_t n_tensors, int64_t n_elems) {
  (void)n_elems;
  return align_up((size_t)n_tensors * sizeof(float), 256) + align_up((size_t)n_tensors * sizeof(double), 256);
}

static int novograd_step_impl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* offsets,
                              int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2, float eps,
                              float weight_decay, float grad_scale, void* workspace, size_t workspace_bytes, void* stream, bool zeroed,
                              float* ema = nullptr, void* ema_state = nullptr, void* clip_state = nullptr);

extern "C" int lasr_novograd_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* offsets,
                                  int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2, float eps,
                                  float weight_decay, float grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
  return novograd_step_impl(params, grads, exp_avg, exp_avg_sq, offsets, n_tensors, n_elems, lr, beta1, beta2, eps, weight_decay, grad_scale,
                            workspace, workspace_bytes, stream, false);
}
// the same step on a workspace the caller keeps: zero before its FIRST use, left zero by every call (the moment kernel re-zeroes the
// norm accumulators it has consumed) - the per-step memset launch (4.6 us in the cfg2 trace) is the caller's one-time torch.zeros
extern "C" int lasr_novograd_step_keep(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* offsets,
                                       int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2, float eps,
                                       float weight_decay, float grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
  return novograd_step_impl(params, grads, exp_avg, exp_avg_sq, offsets, n_tensors, n_elems, lr, beta1, beta2, eps, weight_decay, grad_scale,
                            workspace, workspace_bytes, stream, true);
}

// the step with the weight EMA folded into its last kernel.  ema == NULL (and no state): lasr_novograd_step (keep_workspace == 0) or
// lasr_novograd_step_keep (!= 0), launch for launch
extern "C" int lasr_novograd_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* offsets,
                                      int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2, float eps,
                                      float weight_decay, float grad_scale, void* workspace, size_t workspace_bytes, void* stream,
                                      float* ema, void* ema_state, int keep_workspace) {
  LASR_CHECK_ARG((ema != nullptr) == (ema_state != nullptr), "lasr_novograd_step_ema: ema and ema_state come together (ema %s, state %s)",
                 ema ? "given" : "null", ema_state ? "given" : "null");
  return novograd_step_impl(params, grads, exp_avg, exp_avg_sq, offsets, n_tensors, n_elems, lr, beta1, beta2, eps, weight_decay, grad_scale,
                            workspace, workspace_bytes, stream, keep_workspace != 0, ema, ema_state);
}

// the step with a clip record ("Gradient clipping and the non-finite guard").  clip_state == NULL: lasr_novograd_step_ema, launch
// for launch
extern "C" int lasr_novograd_step_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* offsets,
                                       int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2, float eps,
                                       float weight_decay, float grad_scale, void* workspace, size_t workspace_bytes, void* stream,
                                       float* ema, void* ema_state, int keep_workspace, void* clip_state) {
  LASR_CHECK_ARG((ema != nullptr) == (ema_state != nullptr), "lasr_novograd_step_clip: ema and ema_state come together (ema %s, state %s)",
                 ema ? "given" : "null", ema_state ? "given" : "null");
  return novograd_step_impl(params, grads, exp_avg, exp_avg_sq, offsets, n_tensors, n_elems, lr, beta1, beta2, eps, weight_decay, grad_scale,
                            workspace, workspace_bytes, stream, keep_workspace != 0, ema, ema_state, clip_state);
}

static int novograd_step_impl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* offsets,
                              int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2, float eps,
                              float weight_decay, float grad_scale, void* workspace, size_t workspace_bytes, void* stream, bool zeroed,
                              float* ema, void* ema_state, void* clip_state) {
  LASR_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && offsets && lr && workspace, "lasr_novograd_step: null pointer");
  LASR_CHECK_SHAPE(n_tensors > 0 && n_tensors < (1 << 20) && n_elems > 0, "lasr_novograd_step: n_tensors=%lld", (long long)n_tensors);
  if (ema) {   // the average may overlap none of the buffers the update kernel reads and writes in the same pass
    const float* others[3] = {params, grads, exp_avg};
    for (const float* o : others)
      LASR_CHECK_ARG(ema + n_elems <= o || o + n_elems <= ema, "lasr_novograd_step_ema: ema aliases params, grads or exp_avg");
  }
  if (workspace_bytes < lasr_novograd_workspace_bytes(n_tensors, n_elems)) return fail(LASR_E_WORKSPACE, "lasr_novograd_step: workspace");
  float* denom = reinterpret_cast<float*>(workspace);
  double* norm2 = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + align_up((size_t)n_tensors * sizeof(float), 256));
  hipStream_t st = as_stream(stream);
  // (bench.py's class table) gradients read twice, parameters and momentum read and written
  const int tok = prof_begin(LASR_PROF_OTHER, st, 0.0, 6.0 * (double)n_elems * sizeof(float));
  struct End { int t; hipStream_t s; ~End() { prof_end(t, s); } } end_{tok, st};
  if (!zeroed) {
    hipError_t me = hipMemsetAsync(norm2, 0, (size_t)n_tensors * sizeof(double), st);
    if (me != hipSuccess) return hip_fail(me, "lasr_novograd_step memset");
  }
  ClipState* cst = reinterpret_cast<ClipState*>(clip_state);
  if (cst)
    hipLaunchKernelGGL(novograd_norm_kernel_clip, dim3((unsigned)cdiv(n_elems, kNormChunk)), dim3(256), 0, st, grads, offsets,
                       (int)n_tensors, n_elems, norm2, grad_scale, cst);
  else
    hipLaunchKernelGGL(novograd_norm_kernel, dim3((unsigned)cdiv(n_elems, kNormChunk)), dim3(256), 0, st, grads, offsets, (int)n_tensors,
                       n_elems, norm2, grad_scale);
  LASR_LAUNCH_CHECK("novograd_norm_kernel");
  EmaState* est = reinterpret_cast<EmaState*>(ema_state);
  if (cst && ema)          // one workgroup: the global norm needs every tensor's sum before any is zeroed
    hipLaunchKernelGGL(novograd_moment_kernel_clip<true>, dim3(1), dim3(256), 0, st, norm2, exp_avg_sq, denom, (int)n_tensors, beta2, eps,
                       est, cst);
  else if (cst)
    hipLaunchKernelGGL(novograd_moment_kernel_clip<false>, dim3(1), dim3(256), 0, st, norm2, exp_avg_sq, denom, (int)n_tensors, beta2, eps,
                       est, cst);
  else if (ema)
    hipLaunchKernelGGL(novograd_moment_kernel<true>, dim3((unsigned)cdiv(n_tensors, 256)), dim3(256), 0, st, norm2, exp_avg_sq, denom,
                       (int)n_tensors, beta2, eps, est);
  else
    hipLaunchKernelGGL(novograd_moment_kernel<false>, dim3((unsigned)cdiv(n_tensors, 256)), dim3(256), 0, st, norm2, exp_avg_sq, denom,
                       (int)n_tensors, beta2, eps, est);
  LASR_LAUNCH_CHECK("novograd_moment_kernel");
  int64_t blocks = cdiv(cdiv(n_elems, 4), 256);
  if (blocks > 256 * 8) blocks = 256 * 8;
  const size_t off_bytes = (size_t)(n_tensors + 1) * sizeof(int64_t);
  LASR_CHECK_SHAPE(off_bytes <= 48 * 1024, "lasr_novograd_step: offset table too large for LDS (%lld tensors)", (long long)n_tensors);
  if (cst && ema)
    hipLaunchKernelGGL(novograd_update_kernel_clip<true>, dim3((unsigned)blocks), dim3(256), off_bytes, st, params, grads, exp_avg, offsets,
                       (int)n_tensors, denom, lr, beta1, weight_decay, grad_scale, n_elems, ema, est, cst);
  else if (cst)
    hipLaunchKernelGGL(novograd_update_kernel_clip<false>, dim3((unsigned)blocks), dim3(256), off_bytes, st, params, grads, exp_avg, offsets,
                       (int)n_tensors, denom, lr, beta1, weight_decay, grad_scale, n_elems, ema, est, cst);
  else if (ema)
    hipLaunchKernelGGL(novograd_update_kernel<true>, dim3((unsigned)blocks), dim3(256), off_bytes, st, params, grads, exp_avg, offsets,
                       (int)n_tensors, denom, lr, beta1, weight_decay, grad_scale, n_elems, ema, est);
  else
    hipLaunchKernelGGL(novograd_update_kernel<false>, dim3((unsigned)blocks), dim3(256), off_bytes, st, params, grads, exp_avg, offsets,
                       (int)n_tensors, denom, lr, beta1, weight_decay, grad_scale, n_elems, ema, est);
  LASR_LAUNCH_CHECK("novograd_update_kernel");
  return 0;
}

extern "C" size_t lasr_clip_state_bytes(void) { return sizeof(ClipState); }

// host only: fills a HOST image of the record (the caller uploads it), like lasr_ema_state_init
extern "C" int lasr_clip_state_init(void* host_buf, size_t bytes, int mode, float clip_val, int skip_nonfinite, int64_t steps,
                                    int64_t skipped) {
  LASR_CHECK_ARG(host_buf && bytes >= sizeof(ClipState), "lasr_clip_state_init: buffer of %zu bytes needed", sizeof(ClipState));
  LASR_CHECK_ARG(mode == kClipOff || mode == kClipNorm || mode == kClipValue, "lasr_clip_state_init: mode %d (0 off, 1 norm, 2 value)", mode);
  LASR_CHECK_ARG(clip_val >= 0.f && clip_val <= FLT_MAX, "lasr_clip_state_init: clip_val has to be finite and >= 0, got %g",
                 (double)clip_val);   // (NaN fails both)
  LASR_CHECK_ARG(mode == kClipOff || clip_val > 0.f, "lasr_clip_state_init: mode %d needs clip_val > 0", mode);
  LASR_CHECK_ARG(steps >= 0 && skipped >= 0, "lasr_clip_state_init: steps=%lld skipped=%lld", (long long)steps,
                 (long long)skipped);
  ClipState s;
  memset(&s, 0, sizeof(s));
  s.steps = steps;
  s.skipped = skipped;
  s.mode = mode;
  s.clip_val = clip_val;
  s.skip_nonfinite = skip_nonfinite != 0;
  s.total_norm = 0.f;          // the last step's three: written by every step
  s.coef = 1.f;
  s.last_skipped = 0;
  memcpy(host_buf, &s, sizeof(s));
  return 0;
}

extern "C" size_t lasr_ema_state_bytes(void) { return sizeof(EmaState); }

// host only: fills a HOST image of the record (the caller uploads it), like lasr_lr_schedule_init
extern "C" int lasr_ema_state_init(void* host_buf, size_t bytes, float decay, int warmup, int64_t num_updates) {
  LASR_CHECK_ARG(host_buf && bytes >= sizeof(EmaState), "lasr_ema_state_init: buffer of %zu bytes needed", sizeof(EmaState));
  LASR_CHECK_ARG(decay >= 0.f && decay < 1.f, "lasr_ema_state_init: decay has to be in [0, 1), got %g", (double)decay);   // (NaN fails both)
  LASR_CHECK_ARG(num_updates >= 0, "lasr_ema_state_init: num_updates=%lld", (long long)num_updates);
  EmaState s;
  memset(&s, 0, sizeof(s));
  s.num_updates = num_updates;
  s.decay = decay;
  s.warmup = warmup != 0;
  s.w = 0.f;                   // written by every step before it is read
  memcpy(host_buf, &s, sizeof(s));
  return 0;
}

extern "C" int lasr_ema_update(float* ema, const float* params, int64_t n, float w, void* stream) {
  LASR_CHECK_ARG(ema && params, "lasr_ema_update: null pointer");
  LASR_CHECK_ARG(n >= 0, "lasr_ema_update: n=%lld", (long long)n);
  LASR_CHECK_ARG(ema + n <= params || params + n <= ema || n == 0, "lasr_ema_update: ema aliases params");
  if (n == 0) return 0;
  const uintptr_t pe = reinterpret_cast<uintptr_t>(ema), pp = reinterpret_cast<uintptr_t>(params);
  int64_t head = n, nvec = 0;                           // bases not congruent mod 16 bytes: single elements throughout
  if ((pe & 15) == (pp & 15) && (pe & 3) == 0) {
    head = (int64_t)(((16 - (pe & 15)) & 15) >> 2);
    if (head > n) head = n;
    nvec = (n - head) >> 2;
  }
  int64_t blocks = cdiv(nvec + (n - 4 * nvec), 256);
  if (blocks > 256 * 8) blocks = 256 * 8;
  hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), ema, params, n, head, nvec, w);
  LASR_LAUNCH_CHECK("ema_update_kernel");
  return 0;
}

extern "C" int lasr_grad_accumulate_ranges(float* acc, const float* g, const int64_t* lo, const int64_t* hi, int n_ranges, void* stream) {
  LASR_CHECK_ARG(acc && g && lo && hi, "lasr_grad_accumulate_ranges: null pointer");
  LASR_CHECK_ARG(n_ranges >= 0 && n_ranges <= LASR_ACC_MAX_RANGES, "lasr_grad_accumulate_ranges: %d ranges (at most %d)", n_ranges,
                 LASR_ACC_MAX_RANGES);
  for (int i = 0; i < n_ranges; ++i)
    LASR_CHECK_ARG(lo[i] >= 0 && hi[i] >= lo[i], "lasr_grad_accumulate_ranges: range %d = [%lld, %lld)", i, (long long)lo[i], (long long)hi[i]);
  AccRanges r;
  r.n = 0;
  r.first[0] = 0;
  for (int i = 0; i < n_ranges; ++i) {
    const int64_t len = hi[i] - lo[i];
    if (len == 0) continue;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(acc + lo[i]), pg = reinterpret_cast<uintptr_t>(g + lo[i]);
    int64_t head = len, nvec = 0;                       // bases not congruent mod 16 bytes: the whole piece by single elements
    if ((pa & 15) == (pg & 15) && (pa & 3) == 0) {
      head = (int64_t)(((16 - (pa & 15)) & 15) >> 2);
      if (head > len) head = len;
      nvec = (len - head) >> 2;
    }
    const int k = r.n++;
    r.lo[k] = lo[i];
    r.hi[k] = hi[i];
    r.body[k] = lo[i] + head;
    r.nvec[k] = nvec;
    r.first[k + 1] = r.first[k] + nvec + (len - 4 * nvec);
  }
  if (r.n == 0) return 0;
  for (int k = r.n; k < LASR_ACC_MAX_RANGES; ++k) {
    r.lo[k] = r.hi[k] = r.body[k] = r.nvec[k] = 0;
    r.first[k + 1] = r.first[r.n];
  }
  int64_t blocks = cdiv(r.first[r.n], 256);
  if (blocks > 256 * 8) blocks = 256 * 8;
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), acc, g, r);
  LASR_LAUNCH_CHECK("grad_accumulate_kernel");
  return 0;
}

extern "C" int lasr_grad_accumulate(float* acc, const float* g, int64_t n, void* stream) {
  LASR_CHECK_ARG(acc && g, "lasr_grad_accumulate: null pointer");
  LASR_CHECK_ARG(n >= 0, "lasr_grad_accumulate: n=%lld", (long long)n);
  const int64_t lo = 0;
  return lasr_grad_accumulate_ranges(acc, g, &lo, &n, 1, stream);
}

extern "C" int lasr_cast_pad_f32_to_bf16(const float* in, void* out, int64_t rows, int64_t cols, int64_t ld_out, void* stream) {
  LASR_CHECK_ARG(in && out && rows > 0 && cols > 0 && ld_out >= cols, "lasr_cast_pad_f32_to_bf16: bad argument");
  int64_t blocks = cdiv(rows * ld_out, 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(cast_pad_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), in, reinterpret_cast<bf16_t*>(out), rows,
                     cols, ld_out);
  LASR_LAUNCH_CHECK("cast_pad_bf16_kernel");
  return 0;
}

extern "C" int lasr_cast_f32_to_bf16(const float* in, void* out, int64_t n, void* stream) {
  LASR_CHECK_ARG(in && out && n > 0, "lasr_cast_f32_to_bf16: bad argument");
  int64_t blocks = cdiv(n, 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(cast_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), in, reinterpret_cast<bf16_t*>(out), n);
  LASR_LAUNCH_CHECK("cast_bf16_kernel");
  return 0;
}
