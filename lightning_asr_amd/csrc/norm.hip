// Layout, masking-length, BatchNorm (training statistics) and fused BN-apply/residual/activation
// kernels, forward and backward, over channels-last [B][T][C] activations.
// Replaces models/QuartNet.py:33-37 (MaskCNN lengths, BatchNorm1d(eps=1e-3), ReLU) and :74-77
// (residual add + ReLU), plus their autograd backward.  All statistics are f32.
#include "common.h"
#include "reduce_body.h"
#include "se_seqsum.h"
#include "fused.h"
#include "bn_slice.h"
#include "dropout.h"
#include <algorithm>
#include <string.h>

namespace lasr {

// ------------------------------------------------------------------ layout ------------------
// (B, C, T) f32 <-> [B][T][C] T via a 32x32 LDS tile.
template <typename T, bool TO_BTC>
__global__ __launch_bounds__(256) void transpose_kernel(const void* __restrict__ in_, void* __restrict__ out_,
                                                        int64_t C, int64_t Tt) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int64_t c0 = (int64_t)blockIdx.y * 32, t0 = (int64_t)blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  if (TO_BTC) {
    const float* in = reinterpret_cast<const float*>(in_) + (int64_t)b * C * Tt;
    T* out = reinterpret_cast<T*>(out_) + (int64_t)b * C * Tt;
    for (int i = ty; i < 32; i += 8)
      if (c0 + i < C && t0 + tx < Tt) tile[i][tx] = in[(c0 + i) * Tt + t0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
      if (t0 + i < Tt && c0 + tx < C) Elem<T>::st(out + (t0 + i) * C + c0 + tx, tile[tx][i]);
  } else {
    const T* in = reinterpret_cast<const T*>(in_) + (int64_t)b * C * Tt;
    float* out = reinterpret_cast<float*>(out_) + (int64_t)b * C * Tt;
    for (int i = ty; i < 32; i += 8)
      if (t0 + i < Tt && c0 + tx < C) tile[i][tx] = Elem<T>::ld(in + (t0 + i) * C + c0 + tx);
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
      if (c0 + i < C && t0 + tx < Tt) out[(c0 + i) * Tt + t0 + tx] = tile[tx][i];
  }
}

__global__ void mask_lengths_kernel(const float* __restrict__ pct, int64_t B, float Tf, int32_t* __restrict__ lens,
                                    unsigned long long* __restrict__ step_counter) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < B) lens[i] = (int32_t)(Tf * pct[i]);  // f32 product, truncation toward zero (torch .int())
  if (i == 0 && step_counter) *step_counter += 1ull;   // index of this training forward: the dropout masks' counter (dropout.h)
}

// The two launches every training forward starts with - lens = int(T' * pct) (models/QuartNet.py:311) and the bf16 shadow of the
// weights - are independent of each other: one grid (round 4; the last workgroup does the lengths).
// grid: [cast_blocks of the weight shadow | the depthwise tap tables' blocks (fused.h), one 256-entry block each | the lengths]
__global__ __launch_bounds__(256) void mask_lengths_cast_kernel(const float* __restrict__ pct, int64_t B, float Tf, int32_t* __restrict__ lens,
                                                                unsigned long long* __restrict__ step_counter, const float* __restrict__ in,
                                                                bf16_t* __restrict__ out, int64_t n, int cast_blocks, DwTapJobs jobs) {
  if (blockIdx.x == gridDim.x - 1) {                     // workgroup-uniform
    for (int64_t i = threadIdx.x; i < B; i += 256) lens[i] = (int32_t)(Tf * pct[i]);
    if (threadIdx.x == 0 && step_counter) *step_counter += 1ull;
    return;
  }
  if ((int)blockIdx.x >= cast_blocks) {                  // workgroup-uniform: one block of one layer's tap tables
    const int tb = (int)blockIdx.x - cast_blocks;
    int l = 0;
    while (l + 1 < jobs.n && jobs.blk0[l + 1] <= tb) ++l;
    const int e = (tb - jobs.blk0[l]) * 256 + (int)threadIdx.x;
    if (e < 2 * jobs.C[l] * kDwTapRow) jobs.out[l][e] = dw_tap_entry(jobs.w[l], jobs.C[l], jobs.k[l], e);
    return;
  }
  const int64_t n4 = n >> 2;                             // 16-byte loads, 8-byte stores (the buffers are 256-byte aligned)
  const int64_t stride = (int64_t)cast_blocks * 256;
  for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < n4; e += stride) {
    const float4 v = reinterpret_cast<const float4*>(in)[e];
    uint2 o;
    o.x = (uint32_t)f32_to_bf16(v.x) | ((uint32_t)f32_to_bf16(v.y) << 16);
    o.y = (uint32_t)f32_to_bf16(v.z) | ((uint32_t)f32_to_bf16(v.w) << 16);
    reinterpret_cast<uint2*>(out)[e] = o;
  }
  if (blockIdx.x == 0)
    for (int64_t e = (n4 << 2) + threadIdx.x; e < n; e += 256) out[e] = f32_to_bf16(in[e]);
}

// ------------------------------------------------------------------ BN finalize --------------
// (bn_finalize_channel: bn_slice.h)
__global__ void bn_finalize_kernel(const float* __restrict__ stats, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                                   float* __restrict__ coef, float* __restrict__ saved, int64_t C, float n, float eps,
                                   float momentum, int training) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= C) return;
  bn_finalize_channel(training ? stats[c] : 0.f, training ? stats[C + c] : 0.f, c, gamma, beta, rmean, rvar, coef, saved, C, n, eps,
                      momentum, training);
}

// eval mode: the coefficients of up to 64 BN layers from their running statistics in ONE launch (an eval forward issued
// one tiny launch per layer: 28 x ~5 us of pure latency for the 15 units of the plain model)
struct BnEvalMany { lasr_bn_eval_desc d[64]; };
__global__ __launch_bounds__(256) void bn_eval_coef_many_kernel(BnEvalMany a, float eps) {
  const lasr_bn_eval_desc q = a.d[blockIdx.y];
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= q.C) return;
  bn_finalize_channel(0.f, 0.f, c, q.gamma, q.beta, const_cast<float*>(q.running_mean), const_cast<float*>(q.running_var), q.coef, nullptr,
                      q.C, 1.f, eps, 0.f, 0);
}

// ------------------------------------------------------------------ fixed-order partial sums ----
// (partial_lane_sum: bn_slice.h)
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partials, int n_part, int64_t ncols,
                                                              float* __restrict__ out0, int64_t split, float* __restrict__ out1) {
  __shared__ double s_acc[8][33];
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int64_t c = (int64_t)blockIdx.x * 32 + cl;
  s_acc[pl][cl] = c < ncols ? partial_lane_sum(partials, n_part, ncols, c, pl) : 0.0;
  __syncthreads();
  if (pl == 0 && c < ncols) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += s_acc[i][cl];
    if (c < split) out0[c] = (float)s;
    else if (out1) out1[c - split] = (float)s;
  }
}

// GEMM-epilogue BN partial sums ([tile][sum | sumsq][C]) -> training-mode BN coefficients, for the main
// and the residual branch of a unit in ONE launch (blockIdx.y = branch): the fixed-order f64 column
// reduction of reduce_partials_kernel and the arithmetic of bn_finalize_kernel, without the f32 round
// trip of the statistics through HBM and without three of the four launches.
// (BnBranch / BnBranch2: bn_slice.h)
__global__ __launch_bounds__(256) void bn_finalize_partials_kernel(BnBranch2 br, int64_t C, float n, float eps, float momentum) {
  // block = 16 channels x {sum, sumsq} = 32 columns x 8 partial lanes (the parallelism of reduce_partials_kernel)
  __shared__ double s_acc[8][33];
  const BnBranch& b = blockIdx.y ? br.b[1] : br.b[0];
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int64_t c = (int64_t)blockIdx.x * 16 + (cl & 15);
  s_acc[pl][cl] = c < C ? partial_lane_sum(b.partials, b.n_part, 2 * C, (int64_t)(cl >> 4) * C + c, pl) : 0.0;
  __syncthreads();
  if (pl == 0 && cl < 16 && c < C) {
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { s += s_acc[i][cl]; q += s_acc[i][16 + cl]; }
    if (b.stats) { b.stats[c] = (float)s; b.stats[C + c] = (float)q; }
    bn_finalize_channel((float)s, (float)q, c, b.gamma, b.beta, b.rmean, b.rvar, b.coef, b.saved, C, n, eps, momentum, 1);
  }
}

// The same finalize with the SE squeeze of the unit's y in its grid (ContextSE units, round 4): the first nf workgroups are the
// finalize's, the rest seqsum_vec_kernel's - two launch-floor kernels of the forward chain (4.9 us each) that do not depend on each
// other become one.
template <typename T>
__global__ __launch_bounds__(256) void bn_finalize_seqsum_kernel(BnBranch2 br, int64_t C, float n, float eps, float momentum, int nfx, int nf,
                                                                 const T* __restrict__ x, int Tt, int gx, float* __restrict__ sums) {
  constexpr int RL = 256 / (64 / Vec<T>::kN);
  __shared__ double s_acc[8][33];
  __shared__ float s_red[RL][65];
  if ((int)blockIdx.x < nf) {                              // workgroup-uniform
    const int fx = blockIdx.x % nfx, fy = blockIdx.x / nfx;
    const BnBranch& b = fy ? br.b[1] : br.b[0];
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int64_t c = (int64_t)fx * 16 + (cl & 15);
    s_acc[pl][cl] = c < C ? partial_lane_sum(b.partials, b.n_part, 2 * C, (int64_t)(cl >> 4) * C + c, pl) : 0.0;
    __syncthreads();
    if (pl == 0 && cl < 16 && c < C) {
      double s = 0.0, q = 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i) { s += s_acc[i][cl]; q += s_acc[i][16 + cl]; }
      if (b.stats) { b.stats[c] = (float)s; b.stats[C + c] = (float)q; }
      bn_finalize_channel((float)s, (float)q, c, b.gamma, b.beta, b.rmean, b.rvar, b.coef, b.saved, C, n, eps, momentum, 1);
    }
    return;
  }
  const int id = blockIdx.x - nf;
  seqsum_vec_body<T>(x, Tt, (int)C, sums, id % gx, id / gx, s_red);
}

int bn_finalize_partials_seqsum(const lasr_bn_branch* branches, int n_branches, int64_t C, int64_t n_rows, float eps, float momentum,
                                const void* x, int dtype, int64_t B, int64_t T_, float* sums, void* stream) {
  static const bool off = getenv("LASR_SE_SEQSUM_IN_FINALIZE") && atoi(getenv("LASR_SE_SEQSUM_IN_FINALIZE")) == 0;
  const int v = dtype == LASR_F32 ? 4 : 8;
  if (off || C % v != 0 || reinterpret_cast<uintptr_t>(x) % 16 != 0 || T_ >= ((int64_t)1 << 30) || C >= ((int64_t)1 << 30) || B >= 65536) return 1;
  LASR_CHECK_ARG(branches && n_branches >= 1 && n_branches <= 2 && C > 0 && n_rows > 0 && x && sums, "bn_finalize_partials_seqsum: bad argument");
  BnBranch2 br;
  for (int i = 0; i < 2; ++i) {
    const lasr_bn_branch& q = branches[i < n_branches ? i : 0];
    LASR_CHECK_ARG(q.partials && q.n_partials > 0 && q.gamma && q.beta && q.coef, "bn_finalize_partials_seqsum: null pointer");
    br.b[i] = {q.partials, q.n_partials, q.gamma, q.beta, q.running_mean, q.running_var, q.coef, q.saved, q.stats};
  }
  const int nfx = (int)cdiv(C, 16), nf = nfx * n_branches, gx = (int)cdiv(C, 64);
  const unsigned grid = (unsigned)(nf + gx * B);
  if (dtype == LASR_F32)
    hipLaunchKernelGGL(bn_finalize_seqsum_kernel<float>, dim3(grid), dim3(256), 0, as_stream(stream), br, C, (float)n_rows, eps, momentum, nfx, nf,
                       (const float*)x, (int)T_, gx, sums);
  else
    hipLaunchKernelGGL(bn_finalize_seqsum_kernel<bf16_t>, dim3(grid), dim3(256), 0, as_stream(stream), br, C, (float)n_rows, eps, momentum, nfx, nf,
                       (const bf16_t*)x, (int)T_, gx, sums);
  LASR_LAUNCH_CHECK("bn_finalize_seqsum_kernel");
  return 0;
}

int launch_reduce_partials(const float* partials, int n_part, int64_t ncols, float* out0, int64_t split, float* out1,
                           hipStream_t st) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)cdiv(ncols, 32)), dim3(256), 0, st, partials, n_part, ncols, out0, split, out1);
  LASR_LAUNCH_CHECK("reduce_partials_kernel");
  return 0;
}

// ------------------------------------------------------------------ BN apply + add + act -----
// Thread = one 16-byte column vector (4 f32 / 8 bf16 channels) walking a slab of rows, so the
// per-channel coefficients are fetched once and every access is a full 16 B per lane.
static constexpr int kRowsPerBlock = 32;  // rows per workgroup, backward statistics

// d(act)/d(pre-activation)
__device__ __forceinline__ float act_grad(float p, int act) {
  if (act == LASR_ACT_RELU) return p > 0.f ? 1.f : 0.f;
  if (act == LASR_ACT_SWISH) {
    const float s = 1.f / (1.f + __expf(-p));
    return s * (1.f + p * (1.f - s));
  }
  return 1.f;
}

struct ColGeom { int cv, col_threads, row_lanes, cl, rl; };
template <int V>
__device__ __forceinline__ ColGeom col_geom(int C) {
  ColGeom g;
  g.cv = (int)(C / V);
  g.col_threads = g.cv < 256 ? g.cv : 256;
  g.row_lanes = 256 / g.col_threads;
  g.cl = threadIdx.x % g.col_threads;
  g.rl = threadIdx.x / g.col_threads;
  return g;
}

// Flat streaming form of the two element-wise BN kernels: a workgroup owns a slab of kSlabRows rows, keeps
// the per-channel constants of the whole row in LDS (copied once with 16-byte loads) and its 256 threads
// walk the slab's 16-byte vectors row-major, two vectors in flight per thread.  Registers stay small
// (no per-thread coefficient arrays), so 6-8 waves per SIMD keep enough loads in flight.
static constexpr int kSlabRows = 16;     // backward apply (40*C-byte table per slab)
static constexpr int kFwdSlabRows = 8;   // forward (16*C-byte table per slab)

__device__ __forceinline__ void lds_vec8(const float* p, float (&o)[8]) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  o[0] = lo.x; o[1] = lo.y; o[2] = lo.z; o[3] = lo.w; o[4] = hi.x; o[5] = hi.y; o[6] = hi.z; o[7] = hi.w;
}
__device__ __forceinline__ void lds_vec8(const float* p, float (&o)[4]) {
  const float4 lo = *reinterpret_cast<const float4*>(p);
  o[0] = lo.x; o[1] = lo.y; o[2] = lo.z; o[3] = lo.w;
}

// LDS tables of per-channel constants, [q][C] f32.  A bf16 lane owns 8 consecutive channels = two float4: read
// straight from a linear table the lanes' addresses are 32 B apart and every 16-byte read is a 2-way bank
// conflict (measured: 42-47 % of the LDS cycles of these kernels).  So each table row is stored as two planes -
// the low float4 of every channel octet, then the high float4 - and both reads are unit-stride.  (f32 lanes own
// 4 channels: the linear layout is already unit-stride.)
template <int V>
__device__ __forceinline__ int tab_pos(int i, int C) {        // i: linear index (multiple of 4) into [q][C]
  if (V == 4) return i;
  const int q = i / C, r = i - q * C, j = r >> 2;
  return q * C + ((j & 1) ? (C >> 1) : 0) + ((j >> 1) << 2);
}
__device__ __forceinline__ void tab_vec(const float* row, int c, int C, float (&o)[8]) {   // row = table + q*C
  const float4 lo = *reinterpret_cast<const float4*>(row + (c >> 1));
  const float4 hi = *reinterpret_cast<const float4*>(row + (C >> 1) + (c >> 1));
  o[0] = lo.x; o[1] = lo.y; o[2] = lo.z; o[3] = lo.w; o[4] = hi.x; o[5] = hi.y; o[6] = hi.z; o[7] = hi.w;
}
__device__ __forceinline__ void tab_vec(const float* row, int c, int C, float (&o)[4]) {
  (void)C;
  const float4 lo = *reinterpret_cast<const float4*>(row + c);
  o[0] = lo.x; o[1] = lo.y; o[2] = lo.z; o[3] = lo.w;
}

// V consecutive f32 of a per-(utterance, channel) table (the SE scale / SE gradient) as 16-byte loads, issued together with the
// activation loads (eight scalar loads per vector in the middle of the arithmetic made the SE variants of these kernels 2-3x
// slower: 18.5 / 31.7 / 42.5 us against 8.5 / 14.1 / 15.4 for forward / statistics / apply)
__device__ __forceinline__ void ld_tab(const float* p, float (&o)[8]) { lds_vec8(p, o); }
__device__ __forceinline__ void ld_tab(const float* p, float (&o)[4]) { lds_vec8(p, o); }

// out = act((a*y + b)*se + a2*y2 + b2);  s_tab = [a | b | a2 | b2][C].  Two items per thread in flight, no branch
// around a load (HAS2 is a template parameter, the second item's index is clamped and only its store predicated).
template <typename T, bool HAS2, bool SE, bool DROP>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const T* __restrict__ y, const float* __restrict__ coef,
                                                         const T* __restrict__ y2, const float* __restrict__ coef2,
                                                         const float* __restrict__ se, T* __restrict__ out,
                                                         int rows, int Tt, int C, int act_rt, DropArgs drop) {
  extern __shared__ __attribute__((aligned(16))) float s_tab[];
  constexpr int V = Vec<T>::kN;
  const unsigned long long drop_step = DROP ? *drop.step : 0ull;
  for (int i = threadIdx.x * 4; i < 2 * C; i += 1024) {
    const int d = tab_pos<V>(i, C);
    *reinterpret_cast<float4*>(s_tab + d) = *reinterpret_cast<const float4*>(coef + i);
    *reinterpret_cast<float4*>(s_tab + 2 * C + d) = HAS2 ? *reinterpret_cast<const float4*>(coef2 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  const int cv = C / V;
  const int r0 = blockIdx.x * kFwdSlabRows;
  const int n_items = (min(r0 + kFwdSlabRows, rows) - r0) * cv;
  with_act(act_rt, [&](auto act_c) {
  constexpr int act = decltype(act_c)::value;
  for (int it0 = threadIdx.x; it0 < n_items; it0 += 512) {
    uint4 rv[2], rw[2];
    uint32_t off[2];
    int cc[2], rr[2];
    float sev[2][V];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int it = min(it0 + 256 * u, n_items - 1);
      const int rl = it / cv;
      cc[u] = (it - rl * cv) * V; rr[u] = r0 + rl;
      off[u] = (uint32_t)rr[u] * (uint32_t)C + (uint32_t)cc[u];
      rv[u] = Vec<T>::raw(y + off[u]);
      if (HAS2) rw[u] = Vec<T>::raw(y2 + off[u]);
      if (SE) ld_tab(se + (uint32_t)(rr[u] / Tt) * (uint32_t)C + (uint32_t)cc[u], sev[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = cc[u];
      float v[V], w[V], a[V], b[V], o[V];
      Vec<T>::unpack(rv[u], v);
      tab_vec(s_tab, c, C, a); tab_vec(s_tab + C, c, C, b);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        o[j] = fmaf(v[j], a[j], b[j]);
        if (SE) o[j] *= sev[u][j];
      }
      // nn.Dropout sits at the end of SeprationConv (models/QuartNet.py:38): on the main branch BEFORE the residual add of a
      // block, AFTER the activation of first_cnn / last_cnn2
      float dsc[V];
      if (DROP) drop_scale<V>(drop, drop_step, off[u], dsc);
      if (DROP && HAS2) {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] *= dsc[j];
      }
      if (HAS2) {
        Vec<T>::unpack(rw[u], w);
        tab_vec(s_tab + 2 * C, c, C, a); tab_vec(s_tab + 3 * C, c, C, b);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] += fmaf(w[j], a[j], b[j]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = act_fwd(o[j], act);
      if (DROP && !HAS2) {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] *= dsc[j];
      }
      if (it0 + 256 * u < n_items) Vec<T>::store(out + off[u], o);
    }
  }
  });
}

// pass 1: per-block partial sums -> partials[blk][4][C]  (s1, s2 of branch 1; s1', s2' of branch 2).
// HAS2 is a template parameter and every load is unconditional (clamped row, contribution masked), so there is
// no branch around a load; a thread's rows are taken two at a time with all six 16-byte loads issued before the
// first is unpacked (four at a time, or the constants streamed from LDS, cost the second wave per SIMD:
// measured 34 us against 11).  The kernel was a chain of eight exposed memory round trips per slab.
template <typename T, bool HAS2, bool SE, bool DROP>
__global__ __launch_bounds__(256, 2) void bn_bwd_stats_kernel(const T* __restrict__ dout, const T* __restrict__ y,
                                                              const float* __restrict__ coef, const float* __restrict__ saved,
                                                              const T* __restrict__ y2, const float* __restrict__ coef2,
                                                              const float* __restrict__ saved2, const float* __restrict__ se,
                                                              const float* __restrict__ seg, float* __restrict__ partials,
                                                              int rows, int Tt, int C, int act, DropArgs drop, int per_utt) {
  extern __shared__ __attribute__((aligned(16))) float s_part[];  // [row_lanes][4][C]
  constexpr int V = Vec<T>::kN;
  const unsigned long long drop_step = DROP ? *drop.step : 0ull;
  constexpr int RB = 2;                                           // rows in flight per thread
  const ColGeom g = col_geom<V>(C);
  // per_utt (fused SE + BN backward): slabs do not cross utterances - workgroup (b, slab) - and the sums are those of the gradient
  // at the BN output WITHOUT the SE scale / pooled-path term (per-utterance factors, applied when the slabs are folded)
  int r0 = blockIdx.x * kRowsPerBlock;
  int r1 = min(r0 + kRowsPerBlock, rows);
  if (per_utt) {
    const int nslab = (Tt + kRowsPerBlock - 1) / kRowsPerBlock;
    const int ub = blockIdx.x / nslab, sl = blockIdx.x - ub * nslab;
    r0 = ub * Tt + sl * kRowsPerBlock;
    r1 = min(r0 + kRowsPerBlock, (ub + 1) * Tt);
  }
  if (g.rl < g.row_lanes) {
    for (int cvi = g.cl; cvi < g.cv; cvi += g.col_threads) {
      const int c = cvi * V;
      float a1[V], b1[V], m1[V], q1[V], a2[V], b2[V], m2[V], q2[V];
      lds_vec8(coef + c, a1); lds_vec8(coef + C + c, b1); lds_vec8(saved + c, m1); lds_vec8(saved + C + c, q1);
      if (HAS2) {
        lds_vec8(coef2 + c, a2); lds_vec8(coef2 + C + c, b2); lds_vec8(saved2 + c, m2); lds_vec8(saved2 + C + c, q2);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) a2[j] = b2[j] = m2[j] = q2[j] = 0.f;
      }
      float acc[4][V];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) acc[k][j] = 0.f;
      for (int rb = r0 + g.rl; rb < r1; rb += RB * g.row_lanes) {
        uint4 rd[RB], ry[RB], rr[RB];
        float sev[RB][V], sgv[RB][V];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const uint32_t rowc = (uint32_t)min(rb + i * g.row_lanes, rows - 1);
          const uint32_t off = rowc * (uint32_t)C + (uint32_t)c;
          rd[i] = Vec<T>::raw(dout + off);
          ry[i] = Vec<T>::raw(y + off);
          if (HAS2) rr[i] = Vec<T>::raw(y2 + off);
          if (SE) {
            const uint32_t so = (rowc / (uint32_t)Tt) * (uint32_t)C + (uint32_t)c;
            ld_tab(se + so, sev[i]);
            if (seg) ld_tab(seg + so, sgv[i]);
          }
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          float dvi[V], yvi[V], rvi[V];
          Vec<T>::unpack(rd[i], dvi);
          Vec<T>::unpack(ry[i], yvi);
          if (HAS2) Vec<T>::unpack(rr[i], rvi);
          const int r = rb + i * g.row_lanes;
          const float live = r < r1 ? 1.f : 0.f;                  // rows past the slab contribute nothing
          float dsc[V];
          if (DROP) drop_scale<V>(drop, drop_step, (uint32_t)min(r, rows - 1) * (uint32_t)C + (uint32_t)c, dsc);
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float sej = SE ? sev[i][j] : 1.f;
            const float zm = fmaf(yvi[j], a1[j], b1[j]) * sej * ((DROP && HAS2) ? dsc[j] : 1.f);
            const float z = zm + (HAS2 ? fmaf(rvi[j], a2[j], b2[j]) : 0.f);
            const float d = dvi[j] * act_grad(z, act) * live * ((DROP && !HAS2) ? dsc[j] : 1.f);   // gradient at the pre-activation
            const float dmn = (DROP && HAS2) ? d * dsc[j] : d;                                       // ... reaching the main branch
            const float d1 = per_utt ? dmn : fmaf(dmn, sej, (SE && seg) ? sgv[i][j] * live : 0.f);
            acc[0][j] += d1;
            acc[1][j] = fmaf(d1, (yvi[j] - m1[j]) * q1[j], acc[1][j]);
            if (HAS2) {
              acc[2][j] += d;
              acc[3][j] = fmaf(d, (rvi[j] - m2[j]) * q2[j], acc[3][j]);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) s_part[(g.rl * 4 + k) * C + c + j] = acc[k][j];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * C; i += 256) {
    float s = 0.f;
    for (int l = 0; l < g.row_lanes; ++l) s += s_part[l * 4 * C + i];
    partials[(size_t)blockIdx.x * 4 * C + i] = s;
  }
}

// (pass 2a's per-channel fold, bn_bwd_table_channel, lives in common.h: se.hip's excite-backward kernel ends in it too)
__global__ __launch_bounds__(256) void bn_bwd_table_kernel(const float* __restrict__ coef, const float* __restrict__ saved,
                                                           const float* __restrict__ gamma, const float* __restrict__ sums,
                                                           const float* __restrict__ coef2, const float* __restrict__ saved2,
                                                           const float* __restrict__ gamma2, const float* __restrict__ sums2,
                                                           float inv_n, int C, float* __restrict__ tab, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, float* __restrict__ dgamma2,
                                                           float* __restrict__ dbeta2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const bool has2 = coef2 != nullptr;
  bn_bwd_table_channel(c, C, sums[c], sums[C + c], has2 ? sums2[c] : 0.f, has2 ? sums2[C + c] : 0.f, has2, coef, saved, gamma, coef2,
                       saved2, gamma2, inv_n, tab, dgamma, dbeta, dgamma2, dbeta2);
}

// the same table straight from the unreduced pass-1 partials ([blk][s1 | s2 | s1' | s2'][C]): four f64
// column sums per channel, then the fold (one launch instead of two)
__global__ __launch_bounds__(1024) void bn_bwd_table_partials_kernel(const float* __restrict__ partials, int n_part,
                                                                     const float* __restrict__ coef, const float* __restrict__ saved,
                                                                     const float* __restrict__ gamma, const float* __restrict__ coef2,
                                                                     const float* __restrict__ saved2, const float* __restrict__ gamma2,
                                                                     float inv_n, int C, float* __restrict__ tab,
                                                                     float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                     float* __restrict__ dgamma2, float* __restrict__ dbeta2) {
  // block = 8 channels x 4 sums = 32 columns x 32 partial lanes: the 501 partial rows of a cfg2 unit are ONE batch of 16 loads per
  // thread (with 8 lanes they were four dependent trips to the fabric: 7.2 us per launch)
  __shared__ double s_acc[32][33];
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int c = blockIdx.x * 8 + (cl & 7), k = cl >> 3;
  const bool has2 = coef2 != nullptr;
  s_acc[pl][cl] = (c < C && (k < 2 || has2)) ? partial_lane_sum<32>(partials, n_part, 4 * (int64_t)C, (int64_t)k * C + c, pl) : 0.0;
  __syncthreads();
  if (pl < 4) {                                    // lanes 8*pl .. 8*pl+7 of every column, then the four quarter sums
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += s_acc[pl * 8 + i][cl];
    s_acc[pl * 8][cl] = t;
  }
  __syncthreads();
  if (pl == 0 && cl < 8 && c < C) {
    double t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = (s_acc[0][q * 8 + cl] + s_acc[8][q * 8 + cl]) + (s_acc[16][q * 8 + cl] + s_acc[24][q * 8 + cl]);
    bn_bwd_table_channel(c, C, (float)t[0], (float)t[1], (float)t[2], (float)t[3], has2, coef, saved, gamma, coef2, saved2, gamma2,
                         inv_n, tab, dgamma, dbeta, dgamma2, dbeta2);
  }
}

// pass 2b: dy = G1*d1 + B1*y + C1 (rows past the utterance length zeroed), dy2 = G2*d + B2*y2 + C2.
// Two items per thread in flight, HAS2 a template parameter: no branch around a load.
template <typename T, bool HAS2, bool SE, bool DROP>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dout, const T* __restrict__ y,
                                                           const T* __restrict__ y2, const float* __restrict__ tab,
                                                           const float* __restrict__ se, const float* __restrict__ seg,
                                                           const int32_t* __restrict__ row_lens, T* __restrict__ dy,
                                                           T* __restrict__ dy2, int rows, int Tt, int C, int act, DropArgs drop) {
  extern __shared__ __attribute__((aligned(16))) float s_tab[];  // [10][C]
  constexpr int V = Vec<T>::kN;
  const unsigned long long drop_step = DROP ? *drop.step : 0ull;
  for (int i = threadIdx.x * 4; i < 10 * C; i += 1024) *reinterpret_cast<float4*>(s_tab + tab_pos<V>(i, C)) = *reinterpret_cast<const float4*>(tab + i);
  __syncthreads();
  const int cv = C / V;
  const int r0 = blockIdx.x * kSlabRows;
  const int n_items = (min(r0 + kSlabRows, rows) - r0) * cv;
  for (int it0 = threadIdx.x; it0 < n_items; it0 += 512) {
    uint4 rd[2], ry[2], rr2[2];
    uint32_t off[2];
    int cc[2], rr[2];
    float sev[2][V], sgv[2][V];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int it = min(it0 + 256 * u, n_items - 1);
      const int rl = it / cv;
      cc[u] = (it - rl * cv) * V; rr[u] = r0 + rl;
      off[u] = (uint32_t)rr[u] * (uint32_t)C + (uint32_t)cc[u];
      rd[u] = Vec<T>::raw(dout + off[u]);
      ry[u] = Vec<T>::raw(y + off[u]);
      if (HAS2) rr2[u] = Vec<T>::raw(y2 + off[u]);
      if (SE) {
        const uint32_t so = (uint32_t)(rr[u] / Tt) * (uint32_t)C + (uint32_t)cc[u];
        ld_tab(se + so, sev[u]);
        if (seg) ld_tab(seg + so, sgv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = cc[u], r = rr[u];
      const bool live = it0 + 256 * u < n_items;
      float dv[V], yv[V], rv[V], o1[V], o2[V];
      Vec<T>::unpack(rd[u], dv);
      Vec<T>::unpack(ry[u], yv);
      if (HAS2) Vec<T>::unpack(rr2[u], rv);
      const int ub = r / Tt;
      const bool masked = row_lens && (r - ub * Tt) >= row_lens[ub];
      float a1[V], b1[V], G[V], Bc[V], Cc[V];
      tab_vec(s_tab, c, C, a1); tab_vec(s_tab + C, c, C, b1);
      float z[V];
#pragma unroll
      for (int j = 0; j < V; ++j) z[j] = fmaf(yv[j], a1[j], b1[j]) * (SE ? sev[u][j] : 1.f);
      float dsc[V];
      if (DROP) drop_scale<V>(drop, drop_step, off[u], dsc);
      if (DROP && HAS2) {
#pragma unroll
        for (int j = 0; j < V; ++j) z[j] *= dsc[j];
      }
      if (HAS2) {
        tab_vec(s_tab + 5 * C, c, C, a1); tab_vec(s_tab + 6 * C, c, C, b1);
#pragma unroll
        for (int j = 0; j < V; ++j) z[j] += fmaf(rv[j], a1[j], b1[j]);
      }
      float d[V];
#pragma unroll
      for (int j = 0; j < V; ++j) d[j] = dv[j] * act_grad(z[j], act) * ((DROP && !HAS2) ? dsc[j] : 1.f);
      tab_vec(s_tab + 2 * C, c, C, G); tab_vec(s_tab + 3 * C, c, C, Bc); tab_vec(s_tab + 4 * C, c, C, Cc);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d1 = fmaf((DROP && HAS2) ? d[j] * dsc[j] : d[j], SE ? sev[u][j] : 1.f, (SE && seg) ? sgv[u][j] : 0.f);
        o1[j] = masked ? 0.f : fmaf(G[j], d1, fmaf(Bc[j], yv[j], Cc[j]));
      }
      if (live) Vec<T>::store(dy + off[u], o1);
      if (HAS2) {
        tab_vec(s_tab + 7 * C, c, C, G); tab_vec(s_tab + 8 * C, c, C, Bc); tab_vec(s_tab + 9 * C, c, C, Cc);
#pragma unroll
        for (int j = 0; j < V; ++j) o2[j] = fmaf(G[j], d[j], fmaf(Bc[j], rv[j], Cc[j]));
        if (live) Vec<T>::store(dy2 + off[u], o2);
      }
    }
  }
}



// ---- channel-sliced BN backward (bf16, residual or plain units without SE / dropout) -----------------------------------------
// The row-major pair above needs a launch between its passes that folds 501 partial rows into per-channel constants, because a
// workgroup that walks whole rows needs the constants of ALL channels.  Here a workgroup owns a SLICE of 64 channels (128 bytes of
// every row: whole cache lines) and a chunk of rows, so the statistics pass leaves only `nchunk` partial rows per channel and
// every workgroup of the apply pass folds the constants of its own 64 channels in its prologue (nchunk x 4 x 64 floats from L2):
// statistics -> apply, nothing in between.  block = 8 column threads (16 bytes each) x 64 row lanes.
static constexpr int kSlCh = 64, kSlThreads = 512, kSlLanes = 64;

// An empty volatile statement that reads and writes the values in place: the compiler can move no use of them across it, and keeps
// such statements in program order.
__device__ __forceinline__ void pin_regs(float (&a)[8]) {
  asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]));
}
__device__ __forceinline__ void pin_regs(uint4& v) {
  typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
  u32x4_t t = {v.x, v.y, v.z, v.w};
  asm volatile("" : "+v"(t));
  v = make_uint4(t.x, t.y, t.z, t.w);
}

// SE (ContextSE units): a chunk is one utterance (rpc = T'), so the excite scale of the thread's 8 channels is a register constant
// and the partial rows ARE the per-utterance sums P[b][4][C] the excite backward starts from (sums of the gradient at the BN
// output without the SE factors, as bn_bwd_stats_kernel(per_utt)).
// RB: rows in flight per thread.  ONE: the chunk holds at most RB rows per row lane (the launcher checks), so there is no row loop:
// every lane asks for the coefficient vectors and all of its RB rows at entry - clamped addresses, no branch around a load - and
// no later request waits for an earlier answer (the waits behind the last load count the rows down in the order they were asked
// for).  The rows are added in the same ascending order as the loop adds them (rb + i * 64), and a row past the
// chunk adds d * 0, so the partial rows are the same bits (LASR_BN_STATS_BATCH, profiles/bn_stats_batch_ab.txt).
template <bool HAS2, bool SE, bool NTL = false, int RB = 4, bool ONE = false>
__global__ __launch_bounds__(512) void bn_bwd_stats_sliced_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ y,
                                                                  const float* __restrict__ coef, const float* __restrict__ saved,
                                                                  const bf16_t* __restrict__ y2, const float* __restrict__ coef2,
                                                                  const float* __restrict__ saved2, const float* __restrict__ se,
                                                                  float* __restrict__ partials, int rows, int C, int act_rt, int rpc) {
  __shared__ float s_red[8][4][kSlCh];
  constexpr int V = 8;
  const int tid = threadIdx.x, cl = tid & 7, rl = tid >> 3, lane = tid & 63, wid = tid >> 6;
  const int c = blockIdx.x * kSlCh + cl * V;
  const int r0 = blockIdx.y * rpc, r1 = min(r0 + rpc, rows);
  float a1[V], b1[V], m1[V], q1[V], a2[V], b2[V], m2[V], q2[V];
  lds_vec8(coef + c, a1); lds_vec8(coef + C + c, b1); lds_vec8(saved + c, m1); lds_vec8(saved + C + c, q1);
  if (HAS2) {
    lds_vec8(coef2 + c, a2); lds_vec8(coef2 + C + c, b2); lds_vec8(saved2 + c, m2); lds_vec8(saved2 + C + c, q2);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) a2[j] = b2[j] = m2[j] = q2[j] = 0.f;
  }
  float sev[V];
  if (SE) lds_vec8(se + (size_t)blockIdx.y * C + c, sev);
  float acc[4][V];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[k][j] = 0.f;
  uint4 rd[RB], ry[RB], rr[RB];
  auto load_rows = [&](int rb) {
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      // ONE: a row past the chunk re-reads the chunk's last row, a line the workgroup fetches anyway, not the next chunk's rows
      const uint32_t off = (uint32_t)min(rb + i * kSlLanes, (ONE ? r1 : rows) - 1) * (uint32_t)C + (uint32_t)c;
      rd[i] = Vec<bf16_t>::raw(dout + off);                     // (written a moment ago by the unit above: default policy)
      ry[i] = Vec<bf16_t>::raw_if_nt<NTL>(y + off);
      if (HAS2) rr[i] = Vec<bf16_t>::raw_if_nt<NTL>(y2 + off);
    }
  };
  auto add_rows = [&](int rb, int act) {
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      // ONE: one row at a time, the raw vectors of the later rows stay packed (unpacked ahead, the 24 rows do not fit 256 registers).
      // The empty statements keep their order: the sums of the rows before, then this row's vectors, which nothing unpacks earlier.
      if (ONE) {
#pragma unroll
        for (int k = 0; k < (HAS2 ? 4 : 2); ++k) pin_regs(acc[k]);
        pin_regs(rd[i]); pin_regs(ry[i]);
        if (HAS2) pin_regs(rr[i]);
      }
      float dvi[V], yvi[V], rvi[V];
      Vec<bf16_t>::unpack(rd[i], dvi);
      Vec<bf16_t>::unpack(ry[i], yvi);
      if (HAS2) Vec<bf16_t>::unpack(rr[i], rvi);
      const float live = rb + i * kSlLanes < r1 ? 1.f : 0.f;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float z = fmaf(yvi[j], a1[j], b1[j]) * (SE ? sev[j] : 1.f) + (HAS2 ? fmaf(rvi[j], a2[j], b2[j]) : 0.f);
        const float d = dvi[j] * act_grad(z, act) * live;
        acc[0][j] += d;
        acc[1][j] = fmaf(d, (yvi[j] - m1[j]) * q1[j], acc[1][j]);
        if (HAS2) {
          acc[2][j] += d;
          acc[3][j] = fmaf(d, (rvi[j] - m2[j]) * q2[j], acc[3][j]);
        }
      }
    }
  };
  if constexpr (ONE) {
    // the activation is chosen once, behind the loads: a runtime `act` inside the rows puts a branch around every element, and
    // the values that live across those blocks spill
    const int rb = r0 + rl;
    load_rows(rb);
    if (act_rt == LASR_ACT_RELU) add_rows(rb, LASR_ACT_RELU);
    else if (act_rt == LASR_ACT_SWISH) add_rows(rb, LASR_ACT_SWISH);
    else add_rows(rb, LASR_ACT_NONE);
  } else {
    // (act stays a runtime value here: as a constant the loop body is one basic block, the scheduler overlaps the four rows further and
    //  the 256-register budget spills - measured equal, 12.0 us either way: the pass waits on memory)
    const int act = act_rt;
    for (int rb = r0 + rl; rb < r1; rb += RB * kSlLanes) { load_rows(rb); add_rows(rb, act); }
  }
  // the wave's 8 row lanes (lane bits 3-5), then the 8 waves through LDS in a fixed order
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float v = acc[k][j];
      v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
      acc[k][j] = v;
    }
  if (lane < 8) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < V; ++j) s_red[wid][k][cl * V + j] = acc[k][j];
  }
  __syncthreads();
  if (tid < 4 * kSlCh) {
    const int k = tid >> 6, ch = tid & 63;
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) t += s_red[w][k][ch];
    partials[((size_t)blockIdx.y * 4 + k) * C + blockIdx.x * kSlCh + ch] = t;
  }
}

// SE: the constants come folded from the excite backward (tab_in [10][C], se_bwd_pool_kernel); d1 = d*se + seg with the
// utterance's scale and pooled-path gradient as register constants (a chunk is one utterance).
// RB: rows in flight per thread; WPE: waves per SIMD the register allocation must leave room for (2 = one 512-thread workgroup per
// CU, 4 = two).
template <bool HAS2, bool SE, int RB = 2, int WPE = 2, bool NTL = false>
__global__ __launch_bounds__(512, WPE) void bn_bwd_apply_sliced_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ y,
                                                                  const bf16_t* __restrict__ y2, const float* __restrict__ partials,
                                                                  int nchunk, const float* __restrict__ tab_in, const float* __restrict__ se,
                                                                  const float* __restrict__ seg, const float* __restrict__ coef,
                                                                  const float* __restrict__ saved,
                                                                  const float* __restrict__ gamma, const float* __restrict__ coef2,
                                                                  const float* __restrict__ saved2, const float* __restrict__ gamma2,
                                                                  float inv_n, const int32_t* __restrict__ row_lens, bf16_t* __restrict__ dy,
                                                                  bf16_t* __restrict__ dy2, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                  float* __restrict__ dgamma2, float* __restrict__ dbeta2, int rows, int Tt,
                                                                  int C, int act_rt, int rpc) {
  __shared__ double s_sum[4][kSlCh];
  __shared__ __attribute__((aligned(16))) float s_tab[10][kSlCh];
  constexpr int V = 8;
  const int tid = threadIdx.x, cl = tid & 7, rl = tid >> 3;
  const int c0 = blockIdx.x * kSlCh;
  if (SE) {
    for (int i = tid; i < 10 * kSlCh; i += kSlThreads) s_tab[i >> 6][i & 63] = tab_in[(size_t)(i >> 6) * C + c0 + (i & 63)];
  } else {
    if (tid < 4 * kSlCh) {                               // waves 0-3: the slice's four sums over the chunks, f64, fixed order
      const int k = tid >> 6, ch = tid & 63;
      double a0 = 0.0, a1 = 0.0;
      if (k < 2 || HAS2) {
        const float* p = partials + (size_t)k * C + c0 + ch;
        for (int q = 0; q < nchunk; q += 16) {
          float v[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float x = p[(size_t)min(q + i, nchunk - 1) * 4 * C];
            v[i] = q + i < nchunk ? x : 0.f;
          }
#pragma unroll
          for (int i = 0; i < 16; i += 2) { a0 += (double)v[i]; a1 += (double)v[i + 1]; }
        }
      }
      s_sum[k][ch] = a0 + a1;
    }
    __syncthreads();
    if (tid < kSlCh) {                                   // the constants of pass 2a (bn_bwd_table_channel), kept in LDS
      const int c = c0 + tid;
      const float s1 = (float)s_sum[0][tid], s2 = (float)s_sum[1][tid];
      {
        const float q = saved[C + c], w = s2 * inv_n, G = gamma[c] * q;
        s_tab[0][tid] = coef[c]; s_tab[1][tid] = coef[C + c]; s_tab[2][tid] = G; s_tab[3][tid] = -G * q * w;
        s_tab[4][tid] = G * (saved[c] * q * w - s1 * inv_n);
        if (blockIdx.y == 0) { dbeta[c] = s1; dgamma[c] = s2; }
      }
      if (HAS2) {
        const float s1b = (float)s_sum[2][tid], s2b = (float)s_sum[3][tid];
        const float q = saved2[C + c], w = s2b * inv_n, G = gamma2[c] * q;
        s_tab[5][tid] = coef2[c]; s_tab[6][tid] = coef2[C + c]; s_tab[7][tid] = G; s_tab[8][tid] = -G * q * w;
        s_tab[9][tid] = G * (saved2[c] * q * w - s1b * inv_n);
        if (blockIdx.y == 0) { dbeta2[c] = s1b; dgamma2[c] = s2b; }
      } else {
#pragma unroll
        for (int k = 5; k < 10; ++k) s_tab[k][tid] = 0.f;
      }
    }
  }
  __syncthreads();
  const int c = c0 + cl * V;
  const int r0 = blockIdx.y * rpc, r1 = min(r0 + rpc, rows);
  float sev[V], sgv[V];
  if (SE) { lds_vec8(se + (size_t)blockIdx.y * C + c, sev); lds_vec8(seg + (size_t)blockIdx.y * C + c, sgv); }
  with_act(act_rt, [&](auto act_c) {
  constexpr int act = decltype(act_c)::value;
  for (int rb = r0 + rl; rb < r1; rb += RB * kSlLanes) {
    uint4 rd[RB], ry[RB], rr2[RB];
    uint32_t off[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      off[u] = (uint32_t)min(rb + u * kSlLanes, rows - 1) * (uint32_t)C + (uint32_t)c;
      rd[u] = Vec<bf16_t>::raw(dout + off[u]);
      ry[u] = Vec<bf16_t>::raw_if_nt<NTL>(y + off[u]);
      if (HAS2) rr2[u] = Vec<bf16_t>::raw_if_nt<NTL>(y2 + off[u]);
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int r = rb + u * kSlLanes;
      const bool live = r < r1;
      const int rc = min(r, rows - 1);
      float dv[V], yv[V], rv[V], o1[V], o2[V];
      Vec<bf16_t>::unpack(rd[u], dv);
      Vec<bf16_t>::unpack(ry[u], yv);
      if (HAS2) Vec<bf16_t>::unpack(rr2[u], rv);
      const int ub = rc / Tt;
      const bool masked = row_lens && (rc - ub * Tt) >= row_lens[ub];
      float ca[V], cb[V], G[V], Bc[V], Cc[V], z[V], d[V];
      lds_vec8(&s_tab[0][cl * V], ca); lds_vec8(&s_tab[1][cl * V], cb);
#pragma unroll
      for (int j = 0; j < V; ++j) z[j] = fmaf(yv[j], ca[j], cb[j]) * (SE ? sev[j] : 1.f);
      if (HAS2) {
        lds_vec8(&s_tab[5][cl * V], ca); lds_vec8(&s_tab[6][cl * V], cb);
#pragma unroll
        for (int j = 0; j < V; ++j) z[j] += fmaf(rv[j], ca[j], cb[j]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) d[j] = dv[j] * act_grad(z[j], act);
      lds_vec8(&s_tab[2][cl * V], G); lds_vec8(&s_tab[3][cl * V], Bc); lds_vec8(&s_tab[4][cl * V], Cc);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d1 = SE ? fmaf(d[j], sev[j], sgv[j]) : d[j];
        o1[j] = masked ? 0.f : fmaf(G[j], d1, fmaf(Bc[j], yv[j], Cc[j]));
      }
      if (live) Vec<bf16_t>::store(dy + off[u], o1);
      if (HAS2) {
        lds_vec8(&s_tab[7][cl * V], G); lds_vec8(&s_tab[8][cl * V], Bc); lds_vec8(&s_tab[9][cl * V], Cc);
#pragma unroll
        for (int j = 0; j < V; ++j) o2[j] = fmaf(G[j], d[j], fmaf(Bc[j], rv[j], Cc[j]));
        if (live) Vec<bf16_t>::store(dy2 + off[u], o2);
      }
    }
  }
  });
}

// ---- channel-sliced BN forward apply (bf16, plain / residual units without SE / dropout) -------------------------------------
// The forward's "statistics -> apply, nothing in between": the unit's 1x1 GEMM leaves per-tile partial sums, and every workgroup
// here - 64 channels x a chunk of rows, the backward pair's geometry - folds the coefficients of its own 64 channels from them in its
// prologue (bn_slice_finalize: the finalize launch's arithmetic, so the same numbers), behind the loads of its first rows.  Row
// chunk 0 leaves coef / saved / stats / the running statistics in memory for the backward.  The element arithmetic is
// bn_act_fwd_kernel's, operation for operation.  block = 8 column threads (16 bytes each) x 64 row lanes, RB rows in flight.
// WPE: waves per SIMD the register allocation leaves room for - with the residual branch the prologue's 64 partial loads in flight
// beside the rows' need more than 128 registers (2: one workgroup per CU, as the backward's statistics pass).
template <bool HAS2, int RB = 4, int WPE = HAS2 ? 2 : 4>
__global__ __launch_bounds__(512, WPE) void bn_act_fwd_sliced_kernel(const bf16_t* __restrict__ y, const bf16_t* __restrict__ y2, BnSliceIn in,
                                                                   bf16_t* __restrict__ out, int rows, int C, int act_rt, int rpc) {
  __shared__ double s_acc[kBnSliceAccBytes / 8];
  __shared__ __attribute__((aligned(16))) float s_tab[kBnSliceTabFloats];
  constexpr int V = 8;
  const int tid = threadIdx.x, cl = tid & 7, rl = tid >> 3;
  const int c0 = blockIdx.x * kSlCh, c = c0 + cl * V;
  const int r0 = blockIdx.y * rpc, r1 = min(r0 + rpc, rows);
  uint4 ry[RB], rr[RB];
  auto load_rows = [&](int base, uint4 (&dy_)[RB], uint4 (&dr_)[RB]) {
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const uint32_t off = (uint32_t)min(base + rl + u * kSlLanes, rows - 1) * (uint32_t)C + (uint32_t)c;
      dy_[u] = Vec<bf16_t>::raw(y + off);
      if (HAS2) dr_[u] = Vec<bf16_t>::raw(y2 + off);
    }
  };
  load_rows(r0, ry, rr);                                  // the chunk's first rows are on their way while the slice is finalized
  bn_slice_finalize<HAS2>(in, C, c0, blockIdx.y == 0, s_acc, s_tab);
  float a[V], b[V], a2[V], b2[V];
  lds_vec8(s_tab + cl * V, a); lds_vec8(s_tab + kBnSliceCh + cl * V, b);
  if (HAS2) { lds_vec8(s_tab + 4 * kBnSliceCh + cl * V, a2); lds_vec8(s_tab + 5 * kBnSliceCh + cl * V, b2); }
  with_act(act_rt, [&](auto act_c) {
  constexpr int act = decltype(act_c)::value;
  for (int base = r0;;) {
    const int nbase = base + RB * kSlLanes;
    const bool more = nbase < r1;                         // workgroup-uniform
    uint4 ny[RB], nr[RB];
    if (more) load_rows(nbase, ny, nr);
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int r = base + rl + u * kSlLanes;
      float v[V], w[V], o[V];
      Vec<bf16_t>::unpack(ry[u], v);
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = fmaf(v[j], a[j], b[j]);
      if (HAS2) {
        Vec<bf16_t>::unpack(rr[u], w);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] += fmaf(w[j], a2[j], b2[j]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = act_fwd(o[j], act);
      if (r < r1) Vec<bf16_t>::store(out + (uint32_t)r * (uint32_t)C + (uint32_t)c, o);
    }
    if (!more) break;
#pragma unroll
    for (int u = 0; u < RB; ++u) { ry[u] = ny[u]; if (HAS2) rr[u] = nr[u]; }
    base = nbase;
  }
  });
}

// A/B switches of the channel-sliced kernels, read once per process (the measurements behind each default stand where it is used)
struct BnSwitches {
  static int env_int(const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; }
  const int sliced = env_int("LASR_BN_SLICED", 256);          // backward pair: workgroups per pass, 0 = the row-major kernels
  const int apply_split = env_int("LASR_BN_APPLY_SPLIT", 2);  // backward apply: its chunks per chunk of the statistics pass
  const int fwd_sliced = env_int("LASR_BN_FWD_SLICED", 0);    // forward apply: workgroups, 0 = the default of 256
  const int stats_batch = env_int("LASR_BN_STATS_BATCH", 1);  // backward statistics: chunks of <= 8 rows per lane in one load batch, 0 = the row loop
};
static const BnSwitches& bn_switches() {
  static const BnSwitches s;
  return s;
}

// rows per chunk of the sliced forward apply: 256 workgroups, one round of the chip - every workgroup re-reads its slice's partial sums,
// so more of them only add L2 traffic (cfg2 rows, us per call at 256 / 512 workgroups: C = 512 plain 7.7 / 8.4, residual 10.7 / 15.3;
// C = 1024 residual 18.6 / 20.8).  LASR_BN_FWD_SLICED=<n> sets the count.  At least one row per row lane in a chunk.
static int bn_fwd_sliced_rpc(int64_t rows, int64_t C) {
  const int forced = bn_switches().fwd_sliced;
  const int target = forced > 0 ? forced : 256;
  const int64_t slices = C / kSlCh;
  const int64_t nchunk = std::max<int64_t>(1, std::min<int64_t>(target / slices, rows / kSlLanes));
  return (int)cdiv(rows, nchunk);
}

// rows per chunk of the sliced pair for this shape (0: take the row-major kernels).  One 512-thread workgroup per CU (the
// statistics kernel holds 222 registers per lane): 256 workgroups measured best at cfg2 (128: 2.339, 192: 2.298, 256: 2.262,
// 384: 2.447, 512: 2.419 ms per step; row-major pair with its table launch: 2.372).  LASR_BN_SLICED=<n> sets the count, 0 disables.
static int bn_sliced_rpc(int dtype, int64_t rows, int64_t C, bool se, bool drop, int per_utt, bool reduced_sums) {
  const int target = bn_switches().sliced;
  if (target <= 0 || dtype != LASR_BF16 || se || drop || per_utt || reduced_sums || C % kSlCh != 0 || rows < 4096) return 0;
  const int64_t slices = C / kSlCh;
  // at least one row per row lane in a chunk: the partial rows ([nchunk][4][C]) then also fit the workspace the row-major pair
  // is sized for ([rows / 32][4][C])
  const int64_t nchunk = std::max<int64_t>(1, std::min<int64_t>(target / slices, rows / kSlLanes));
  return (int)cdiv(rows, nchunk);
}

}  // namespace lasr

using namespace lasr;

// dtype x HAS2 x SE x DROP - the template head of the three row-slab kernels - as four tags inside f
template <typename F>
static void with_bn_variant(int dtype, bool has2, bool se, bool drop, F&& f) {
  with_dtype(dtype, [&](auto t) {
    with_bool(has2, [&](auto h2) { with_bool(se, [&](auto s) { with_bool(drop, [&](auto d) { f(t, h2, s, d); }); }); });
  });
}

extern "C" int lasr_bct_to_btc(const float* in, void* out, int dtype, int64_t B, int64_t C, int64_t T_, void* stream) {
  LASR_CHECK_ARG(in && out && (dtype == LASR_F32 || dtype == LASR_BF16), "lasr_bct_to_btc: bad argument");
  LASR_CHECK_SHAPE(B > 0 && C > 0 && T_ > 0 && B < 65536, "lasr_bct_to_btc: shape");
  dim3 grid((unsigned)cdiv(T_, 32), (unsigned)cdiv(C, 32), (unsigned)B);
  with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL((transpose_kernel<typename decltype(t)::type, true>), grid, dim3(256), 0, as_stream(stream), in, out, C, T_);
  });
  LASR_LAUNCH_CHECK("transpose_kernel");
  return 0;
}
extern "C" int lasr_btc_to_bct(const void* in, int dtype, float* out, int64_t B, int64_t C, int64_t T_, void* stream) {
  LASR_CHECK_ARG(in && out && (dtype == LASR_F32 || dtype == LASR_BF16), "lasr_btc_to_bct: bad argument");
  LASR_CHECK_SHAPE(B > 0 && C > 0 && T_ > 0 && B < 65536, "lasr_btc_to_bct: shape");
  dim3 grid((unsigned)cdiv(T_, 32), (unsigned)cdiv(C, 32), (unsigned)B);
  with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL((transpose_kernel<typename decltype(t)::type, false>), grid, dim3(256), 0, as_stream(stream), in, out, C, T_);
  });
  LASR_LAUNCH_CHECK("transpose_kernel");
  return 0;
}

extern "C" int lasr_mask_lengths_step(const float* pct, int64_t B, int64_t T_, int32_t* lens, uint64_t* step_counter, void* stream) {
  LASR_CHECK_ARG(pct && lens && B > 0 && T_ > 0, "lasr_mask_lengths: bad argument");
  hipLaunchKernelGGL(mask_lengths_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, as_stream(stream), pct, B, (float)T_, lens,
                     reinterpret_cast<unsigned long long*>(step_counter));
  LASR_LAUNCH_CHECK("mask_lengths_kernel");
  return 0;
}
int lasr::mask_lengths_step_cast(const float* pct, int64_t B, int64_t T_, int32_t* lens, uint64_t* step_counter, const float* in, void* out,
                                 int64_t n, const DwTapJobs* jobs, void* stream) {
  LASR_CHECK_ARG(pct && lens && B > 0 && T_ > 0 && in && out && n > 0, "mask_lengths_step_cast: bad argument");
  if (reinterpret_cast<uintptr_t>(in) % 16 || reinterpret_cast<uintptr_t>(out) % 8) return 1;
  int64_t blocks = cdiv(n >> 2, 256);
  if (blocks > 256 * 8) blocks = 256 * 8;
  if (blocks < 1) blocks = 1;
  DwTapJobs j;
  memset(&j, 0, sizeof(j));
  int tap_blocks = 0;
  if (jobs) {
    j = *jobs;
    tap_blocks = j.blk0[j.n];
  }
  hipLaunchKernelGGL(mask_lengths_cast_kernel, dim3((unsigned)(blocks + tap_blocks + 1)), dim3(256), 0, as_stream(stream), pct, B, (float)T_, lens,
                     reinterpret_cast<unsigned long long*>(step_counter), in, reinterpret_cast<bf16_t*>(out), n, (int)blocks, j);
  LASR_LAUNCH_CHECK("mask_lengths_cast_kernel");
  return 0;
}

extern "C" int lasr_mask_lengths(const float* pct, int64_t B, int64_t T_, int32_t* lens, void* stream) {
  return lasr_mask_lengths_step(pct, B, T_, lens, nullptr, stream);
}

// keep[e] = 1 / 0 for the first n elements of the mask a kernel draws for `dropout` at the CURRENT value of its step counter
// (verification: the oracle applies the very same mask)
namespace lasr {
__global__ __launch_bounds__(256) void dropout_mask_kernel(DropArgs d, int64_t n, uint8_t* __restrict__ keep) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v * 8 >= n) return;
  const uint32_t m = d.step ? drop_keep8(d, *d.step, (uint32_t)v) : 0xffu;
  for (int i = 0; i < 8 && v * 8 + i < n; ++i) keep[v * 8 + i] = (m >> i) & 1u;
}
}  // namespace lasr
extern "C" int lasr_dropout_mask(const lasr_dropout* dropout, int64_t n, uint8_t* keep, void* stream) {
  LASR_CHECK_ARG(dropout && keep && n > 0 && n < ((int64_t)1 << 34), "lasr_dropout_mask: bad argument");
  hipLaunchKernelGGL(lasr::dropout_mask_kernel, dim3((unsigned)cdiv(cdiv(n, 8), 256)), dim3(256), 0, as_stream(stream), make_drop(*dropout), n, keep);
  LASR_LAUNCH_CHECK("dropout_mask_kernel");
  return 0;
}

extern "C" int lasr_bn_finalize(const float* stats, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, float* coef, float* saved, int64_t C, int64_t n_rows, float eps,
                                float momentum, int training, void* stream) {
  LASR_CHECK_ARG(gamma && beta && coef && C > 0 && n_rows > 0, "lasr_bn_finalize: bad argument");
  LASR_CHECK_ARG(training ? stats != nullptr : (running_mean && running_var), "lasr_bn_finalize: missing statistics");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, as_stream(stream), stats, gamma, beta,
                     running_mean, running_var, coef, saved, C, (float)n_rows, eps, momentum, training);
  LASR_LAUNCH_CHECK("bn_finalize_kernel");
  return 0;
}

extern "C" int lasr_bn_finalize_partials(const lasr_bn_branch* branches, int n_branches, int64_t C, int64_t n_rows, float eps,
                                         float momentum, void* stream) {
  LASR_CHECK_ARG(branches && (n_branches == 1 || n_branches == 2) && C > 0 && n_rows > 0, "lasr_bn_finalize_partials: bad argument");
  BnBranch2 br;
  for (int i = 0; i < 2; ++i) {
    const lasr_bn_branch& q = branches[i < n_branches ? i : 0];
    LASR_CHECK_ARG(q.partials && q.n_partials > 0 && q.gamma && q.beta && q.coef, "lasr_bn_finalize_partials: null pointer");
    br.b[i] = {q.partials, q.n_partials, q.gamma, q.beta, q.running_mean, q.running_var, q.coef, q.saved, q.stats};
  }
  hipLaunchKernelGGL(bn_finalize_partials_kernel, dim3((unsigned)cdiv(C, 16), (unsigned)n_branches), dim3(256), 0, as_stream(stream), br, C,
                     (float)n_rows, eps, momentum);
  LASR_LAUNCH_CHECK("bn_finalize_partials_kernel");
  return 0;
}

static int check_bn_shape(const char* who, int dtype, int64_t B, int64_t T_, int64_t C) {
  LASR_CHECK_ARG(dtype == LASR_F32 || dtype == LASR_BF16, "%s: bad dtype", who);
  const int v = dtype == LASR_F32 ? 4 : 8;
  LASR_CHECK_SHAPE(C % v == 0 && C <= 4096 && B > 0 && T_ > 0, "%s: C=%lld must be a multiple of %d (16-byte channel vectors)", who,
                   (long long)C, v);
  LASR_CHECK_SHAPE(B * T_ * C < ((int64_t)1 << 31), "%s: tensor exceeds the kernels' 32-bit element offsets", who);
  return 0;
}

// ---- lasr_bn_tail (include/lasr.h): checked once per entry point, unpacked into the kernels' argument lists -------------------------
static bool bn_side_ok(const lasr_bn_side& s, int need) {
  return s.coef && (!(need & kBnSaved) || s.saved) && (!(need & kBnGamma) || s.gamma) && (!(need & kBnBeta) || s.beta) &&
         (!(need & kBnDy) || s.dy) && (!(need & kBnDparams) || (s.dgamma && s.dbeta));
}
int lasr::check_bn_ptrs(const char* who, const lasr_bn_tail* t, int need) {
  LASR_CHECK_ARG(t && t->main.y && bn_side_ok(t->main, need) && (!(need & kBnDout) || t->dout) && (!(need & kBnSeScale) || t->se_scale),
                 "%s: null pointer", who);
  LASR_CHECK_ARG(!t->res.y || (bn_side_ok(t->res, need & ~kBnBeta) && (!(need & kBnSums) || t->res.sums || !t->main.sums)),
                 "%s: branch-2 pointers", who);
  return 0;
}
// `buf`: the entry point's output or workspace
static int check_bn_tail(const char* who, const lasr_bn_tail* t, int need, const void* buf) {
  LASR_TRY(check_bn_ptrs(who, t, need));
  LASR_CHECK_ARG(buf, "%s: null pointer", who);
  return check_bn_shape(who, t->dtype, t->B, t->T, t->C);
}

extern "C" int lasr_bn_act_fwd(const lasr_bn_tail* tail, void* out, void* stream) {
  LASR_TRY(check_bn_tail("lasr_bn_act_fwd", tail, 0, out));
  const lasr_bn_tail& t = *tail;
  const lasr_bn_side r = res_side(t);
  const DropArgs da = make_drop(t.dropout);
  const int64_t rows = t.B * t.T;
  const size_t shmem = (size_t)4 * t.C * sizeof(float);
  with_bn_variant(t.dtype, r.y != nullptr, t.se_scale != nullptr, da.step != nullptr, [&](auto e, auto h2, auto se, auto drop) {
    using T = typename decltype(e)::type;
    hipLaunchKernelGGL((bn_act_fwd_kernel<T, h2.value, se.value, drop.value>), dim3((unsigned)cdiv(rows, kFwdSlabRows)), dim3(256), shmem,
                       as_stream(stream), (const T*)t.main.y, t.main.coef, (const T*)r.y, r.coef, t.se_scale, (T*)out, (int)rows, (int)t.T,
                       (int)t.C, t.act, da);
  });
  LASR_LAUNCH_CHECK("bn_act_fwd_kernel");
  return 0;
}

// host side of BnSliceIn (bn_slice.h): the public branch descriptions of a unit whose finalize is left to its consumer
int lasr::bn_slice_in(const lasr_bn_branch* branches, int n_branches, int64_t n_rows, float eps, float momentum, BnSliceIn* in) {
  LASR_CHECK_ARG(branches && (n_branches == 1 || n_branches == 2) && n_rows > 0 && in, "bn_slice_in: bad argument");
  for (int i = 0; i < 2; ++i) {
    const lasr_bn_branch& q = branches[i < n_branches ? i : 0];
    LASR_CHECK_ARG(q.partials && q.n_partials > 0 && q.gamma && q.beta && q.coef && (!q.running_mean || q.running_var),
                   "bn_slice_in: null pointer");
    in->br.b[i] = {q.partials, q.n_partials, q.gamma, q.beta, q.running_mean, q.running_var, q.coef, q.saved, q.stats};
  }
  in->nb = n_branches; in->n = (float)n_rows; in->eps = eps; in->momentum = momentum;
  return 0;
}

extern "C" int lasr_bn_act_fwd_partials(const lasr_bn_branch* branches, int n_branches, float eps, float momentum, const lasr_bn_tail* tail,
                                        void* out, void* stream) {
  LASR_CHECK_ARG(tail && tail->main.y && out && n_branches == (tail->res.y ? 2 : 1), "lasr_bn_act_fwd_partials: bad argument");
  const void *y = tail->main.y, *y2 = tail->res.y;
  const int64_t C = tail->C, rows = tail->B * tail->T;
  LASR_TRY(check_bn_shape("lasr_bn_act_fwd_partials", tail->dtype, tail->B, tail->T, C));
  LASR_CHECK_SHAPE(tail->dtype == LASR_BF16 && C % kSlCh == 0, "lasr_bn_act_fwd_partials: bf16 and C=%lld a multiple of 64 only", (long long)C);
  LASR_CHECK_ARG(reinterpret_cast<uintptr_t>(y) % 16 == 0 && reinterpret_cast<uintptr_t>(y2) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
                 "lasr_bn_act_fwd_partials: 16-byte alignment");
  BnSliceIn in;
  LASR_TRY(bn_slice_in(branches, n_branches, rows, eps, momentum, &in));
  const int rpc = bn_fwd_sliced_rpc(rows, C);
  const dim3 grid((unsigned)(C / kSlCh), (unsigned)cdiv(rows, rpc));
  with_bool(y2 != nullptr, [&](auto h2) {
    hipLaunchKernelGGL((bn_act_fwd_sliced_kernel<decltype(h2)::value>), grid, dim3(kSlThreads), 0, as_stream(stream), (const bf16_t*)y,
                       (const bf16_t*)y2, in, (bf16_t*)out, (int)rows, (int)C, tail->act, rpc);
  });
  LASR_LAUNCH_CHECK("bn_act_fwd_sliced_kernel");
  return 0;
}

extern "C" size_t lasr_bn_bwd_workspace_bytes(int64_t B, int64_t T_, int64_t C) {
  // pass-1 partials [blk][4][C], then the folded constants [10][C] of pass 2
  return (size_t)cdiv(B * T_, kRowsPerBlock) * 4 * C * sizeof(float) + (size_t)10 * C * sizeof(float);
}

// Pass 1 of a checked tail into `partials`: [ceil(B*T/32)][4][C], or per_utt = 1: [B * ceil(T/32)][4][C] of the raw sums, one
// workgroup per (utterance, 32-frame slab) (see the kernel)
static int bn_bwd_stats_impl(const lasr_bn_tail& t, float* partials, void* stream, int per_utt) {
  const lasr_bn_side &m = t.main, r = res_side(t);
  const DropArgs da = make_drop(t.dropout);
  const int64_t C = t.C, rows = t.B * t.T;
  const int nblk = per_utt ? (int)(t.B * cdiv(t.T, kRowsPerBlock)) : (int)cdiv(rows, kRowsPerBlock);
  if (const int rpc = bn_sliced_rpc(t.dtype, rows, C, t.se_scale != nullptr, da.step != nullptr, per_utt, m.sums != nullptr)) {
    const dim3 grid((unsigned)(C / kSlCh), (unsigned)cdiv(rows, rpc));
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kSlThreads), 0, as_stream(stream), (const bf16_t*)t.dout, (const bf16_t*)m.y, m.coef, m.saved,
                         (const bf16_t*)r.y, r.coef, r.saved, nullptr, partials, (int)rows, (int)C, t.act, rpc);
    };
    // at most 8 rows per row lane (every cfg2 shape but the 1024-channel unit, the 256- and 512-channel shapes of cfg5): one load
    // batch, no row loop.  Up to 4 rows per lane take a batch of 4: in a batch of 8 the four dead rows cost the 256-channel
    // launches 2 us each (profiles/bn_stats_batch_ab.txt)
    const int64_t rpl = cdiv(rpc, kSlLanes);
    const bool one_batch = bn_switches().stats_batch != 0 && (nt_loads_mask() & 1) == 0 && rpl <= 8;
    with_bool(r.y != nullptr, [&](auto h2) {
      constexpr bool H2 = decltype(h2)::value;
      if (one_batch && rpl <= 4) launch(bn_bwd_stats_sliced_kernel<H2, false, false, 4, true>);
      else if (one_batch) launch(bn_bwd_stats_sliced_kernel<H2, false, false, 8, true>);
      else with_bool((nt_loads_mask() & 1) != 0, [&](auto nt) { launch(bn_bwd_stats_sliced_kernel<H2, false, decltype(nt)::value>); });
    });
    LASR_LAUNCH_CHECK("bn_bwd_stats_sliced_kernel");
    return 0;
  }
  const int cv = (int)(C / (t.dtype == LASR_F32 ? 4 : 8));
  const int col_threads = cv < 256 ? cv : 256;
  const int row_lanes = 256 / col_threads;
  const size_t shmem = (size_t)row_lanes * 4 * C * sizeof(float);
  LASR_CHECK_SHAPE(shmem <= 64 * 1024, "lasr_bn_act_bwd_stats: C too large for LDS staging");
  with_bn_variant(t.dtype, r.y != nullptr, t.se_scale != nullptr, da.step != nullptr, [&](auto e, auto h2, auto se, auto drop) {
    using T = typename decltype(e)::type;
    hipLaunchKernelGGL((bn_bwd_stats_kernel<T, h2.value, se.value, drop.value>), dim3(nblk), dim3(256), shmem, as_stream(stream),
                       (const T*)t.dout, (const T*)m.y, m.coef, m.saved, (const T*)r.y, r.coef, r.saved, t.se_scale, t.se_grad, partials,
                       (int)rows, (int)t.T, (int)C, t.act, da, per_utt);
  });
  LASR_LAUNCH_CHECK("bn_bwd_stats_kernel");
  if (!m.sums) return 0;   // partials stay in the workspace for lasr_bn_act_bwd_apply(sums = NULL)
  return launch_reduce_partials(partials, nblk, 4 * C, m.sums, 2 * C, r.sums, as_stream(stream));
}

extern "C" int lasr_bn_act_bwd_stats(const lasr_bn_tail* tail, void* workspace, size_t workspace_bytes, void* stream) {
  LASR_TRY(check_bn_tail("lasr_bn_act_bwd_stats", tail, kBnDout | kBnSaved | kBnSums, workspace));
  if (workspace_bytes < (size_t)cdiv(tail->B * tail->T, kRowsPerBlock) * 4 * tail->C * sizeof(float))
    return fail(LASR_E_WORKSPACE, "lasr_bn_act_bwd_stats: workspace");
  return bn_bwd_stats_impl(*tail, reinterpret_cast<float*>(workspace), stream, 0);
}

extern "C" size_t lasr_bn_bwd_apply_workspace_bytes(int64_t C) { return (size_t)10 * C * sizeof(float); }

// Pass 2 of the channel-sliced pair from the statistics pass's partial rows (chunks of rpc rows) in the workspace
static int launch_bn_bwd_apply_sliced(const lasr_bn_tail& t, int rpc, const float* partials, hipStream_t st) {
  const lasr_bn_side &m = t.main, r = res_side(t);
  const int64_t C = t.C, rows = t.B * t.T;
  const int nchunk = (int)cdiv(rows, rpc);          // partial rows of the statistics pass
  // The apply pass takes row chunks HALF as long as the statistics pass (LASR_BN_APPLY_SPLIT = 2; 1: the same chunks): 512
  // workgroups with one row in flight per thread in 121 registers, so two are resident per CU and their load, arithmetic and
  // store phases interleave - against one round of 256 workgroups that are all in the same phase at the same time.  Measured in
  // the cfg2 step, one call: split 1 / 2 / 3 / 4 = 2.228 / 2.191 / 2.220 / 2.235 ms.  (The statistics pass does not gain from the
  // same treatment: 2.219 with both split against 2.198.)  The arithmetic per element is unchanged.
  const int asplit = bn_switches().apply_split;
  // rb = rows in flight per thread, wpe = workgroups per CU the kernel is bounded for: (1, 4) on the half chunks, (2, 2) on whole ones
  auto launch = [&](auto rb, auto wpe, int rows_per_chunk) {
    const dim3 grid((unsigned)(C / kSlCh), (unsigned)cdiv(rows, rows_per_chunk));
    with_bool(r.y != nullptr, [&](auto h2) {
      with_bool((nt_loads_mask() & 2) != 0, [&](auto nt) {
        constexpr bool H2 = decltype(h2)::value, NT = decltype(nt)::value;
        hipLaunchKernelGGL((bn_bwd_apply_sliced_kernel<H2, false, decltype(rb)::value, decltype(wpe)::value, NT>), grid, dim3(kSlThreads),
                           0, st, (const bf16_t*)t.dout, (const bf16_t*)m.y, (const bf16_t*)r.y, partials, nchunk, nullptr, nullptr, nullptr,
                           m.coef, m.saved, m.gamma, r.coef, r.saved, r.gamma, 1.0f / (float)rows, t.row_lens, (bf16_t*)m.dy,
                           (bf16_t*)r.dy, m.dgamma, m.dbeta, r.dgamma, r.dbeta, (int)rows, (int)t.T, (int)C, t.act, rows_per_chunk);
      });
    });
  };
  const int rpc2 = asplit > 1 ? (int)cdiv(rows, (int64_t)nchunk * asplit) : rpc;
  if (asplit > 1 && rpc2 >= kSlLanes) launch(std::integral_constant<int, 1>{}, std::integral_constant<int, 4>{}, rpc2);
  else launch(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{}, rpc);
  LASR_LAUNCH_CHECK("bn_bwd_apply_sliced_kernel");
  return 0;
}

// Pass 2 of the row-major pair from the folded table: dy = G*(d*se + se_grad) + Bc*y + Cc, dy2 = G2*d + ...  (lasr_bn_act_bwd_apply and
// lasr_bn_se_bwd)
static int launch_bn_bwd_apply(const char* who, const lasr_bn_tail& t, const float* tab, hipStream_t st) {
  const lasr_bn_side r = res_side(t);
  const DropArgs da = make_drop(t.dropout);
  const int64_t rows = t.B * t.T;
  const size_t shmem = (size_t)10 * t.C * sizeof(float);
  LASR_CHECK_SHAPE(shmem <= 64 * 1024, "%s: C too large for the LDS coefficient table", who);
  with_bn_variant(t.dtype, r.y != nullptr, t.se_scale != nullptr, da.step != nullptr, [&](auto e, auto h2, auto se, auto drop) {
    using T = typename decltype(e)::type;
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, h2.value, se.value, drop.value>), dim3((unsigned)cdiv(rows, kSlabRows)), dim3(256), shmem,
                       st, (const T*)t.dout, (const T*)t.main.y, (const T*)r.y, tab, t.se_scale, t.se_grad, t.row_lens, (T*)t.main.dy,
                       (T*)r.dy, (int)rows, (int)t.T, (int)t.C, t.act, da);
  });
  LASR_LAUNCH_CHECK("bn_bwd_apply_kernel");
  return 0;
}

extern "C" int lasr_bn_act_bwd_apply(const lasr_bn_tail* tail, void* workspace, size_t workspace_bytes, void* stream) {
  LASR_TRY(check_bn_tail("lasr_bn_act_bwd_apply", tail, kBnDout | kBnSaved | kBnGamma | kBnDy | kBnSums, workspace));
  const lasr_bn_tail& t = *tail;
  const lasr_bn_side &m = t.main, r = res_side(t);
  const int64_t C = t.C, rows = t.B * t.T;
  hipStream_t st = as_stream(stream);
  if (const int rpc = bn_sliced_rpc(t.dtype, rows, C, t.se_scale != nullptr, make_drop(t.dropout).step != nullptr, 0, m.sums != nullptr)) {
    if (workspace_bytes < lasr_bn_bwd_workspace_bytes(t.B, t.T, C)) return fail(LASR_E_WORKSPACE, "lasr_bn_act_bwd_apply: workspace");
    LASR_CHECK_ARG(m.dgamma && m.dbeta && (!r.y || (r.dgamma && r.dbeta)), "lasr_bn_act_bwd_apply: parameter-gradient pointers");
    return launch_bn_bwd_apply_sliced(t, rpc, reinterpret_cast<const float*>(workspace), st);
  }
  float* tab;
  if (m.sums) {
    if (workspace_bytes < lasr_bn_bwd_apply_workspace_bytes(C)) return fail(LASR_E_WORKSPACE, "lasr_bn_act_bwd_apply: workspace");
    tab = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(bn_bwd_table_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, st, m.coef, m.saved, m.gamma, m.sums, r.coef,
                       r.saved, r.gamma, r.sums, 1.0f / (float)rows, (int)C, tab, m.dgamma, m.dbeta, r.dgamma, r.dbeta);
    LASR_LAUNCH_CHECK("bn_bwd_table_kernel");
  } else {
    // the workspace of the preceding lasr_bn_act_bwd_stats(sums = NULL): unreduced partials, then room for the table
    if (workspace_bytes < lasr_bn_bwd_workspace_bytes(t.B, t.T, C)) return fail(LASR_E_WORKSPACE, "lasr_bn_act_bwd_apply: workspace");
    const int nblk = (int)cdiv(rows, kRowsPerBlock);
    const float* partials = reinterpret_cast<const float*>(workspace);
    tab = reinterpret_cast<float*>(workspace) + (size_t)nblk * 4 * C;
    hipLaunchKernelGGL(bn_bwd_table_partials_kernel, dim3((unsigned)cdiv(C, 8)), dim3(1024), 0, st, partials, nblk, m.coef, m.saved, m.gamma,
                       r.coef, r.saved, r.gamma, 1.0f / (float)rows, (int)C, tab, m.dgamma, m.dbeta, r.dgamma, r.dbeta);
    LASR_LAUNCH_CHECK("bn_bwd_table_partials_kernel");
  }
  return launch_bn_bwd_apply("lasr_bn_act_bwd_apply", t, tab, st);
}

extern "C" size_t lasr_bn_se_bwd_workspace_bytes(int64_t B, int64_t T_, int64_t C) {
  // raw partials [B*ceil(T/32)][4][C] | folded table [10][C] | the excite backward's hand-over (se_bwd_work_bytes)
  return align_up((size_t)B * cdiv(T_, kRowsPerBlock) * 4 * C * sizeof(float), 256) + align_up((size_t)10 * C * sizeof(float), 256) +
         se_bwd_work_bytes(B, C);
}

// Backward of a ContextSE unit's  out = act(BN(y) * se + BN_res(y2))  (models/QuartNetContextSE.py:19-23,54-57) in TWO passes over
// (dout, y, y2) instead of three: per-utterance raw sums -> ds (SE scale gradient) by algebra -> excite-MLP backward (seg, dW1,
// dW2) -> BN-backward constants -> apply.  se.ysum [B][C] = sum_t y of the forward (lasr_seqsum).  se.seg [B][C] is also returned.
extern "C" int lasr_bn_se_bwd(const lasr_bn_tail* tail, const lasr_se_side* se_side, void* workspace, size_t workspace_bytes, void* stream) {
  LASR_TRY(check_bn_tail("lasr_bn_se_bwd", tail, kBnDout | kBnSeScale | kBnSaved | kBnGamma | kBnBeta | kBnDy | kBnDparams, workspace));
  LASR_CHECK_ARG(se_side && se_side->hidden && se_side->pooled && se_side->ysum && se_side->W1 && se_side->W2 && se_side->seg &&
                     se_side->dW1 && se_side->dW2, "lasr_bn_se_bwd: null pointer");
  const lasr_se_side& se = *se_side;
  lasr_bn_tail t = *tail;      // the sums go through the workspace, and pass 1 takes the raw sums: se.seg joins in pass 2
  t.main.sums = t.res.sums = nullptr;
  t.se_grad = nullptr;
  const lasr_bn_side &m = t.main, r = res_side(t);
  const int64_t B = t.B, T_ = t.T, C = t.C;
  if (workspace_bytes < lasr_bn_se_bwd_workspace_bytes(B, T_, C)) return fail(LASR_E_WORKSPACE, "lasr_bn_se_bwd: workspace");
  hipStream_t st = as_stream(stream);
  const int nslab = (int)cdiv(T_, kRowsPerBlock);
  char* w = reinterpret_cast<char*>(workspace);
  float* partials = reinterpret_cast<float*>(w);
  w += align_up((size_t)B * nslab * 4 * C * sizeof(float), 256);
  float* tab = reinterpret_cast<float*>(w);
  w += align_up((size_t)10 * C * sizeof(float), 256);
  void* se_work = w;
  // channel-sliced form: one workgroup per (64 channels, utterance) in both passes - the statistics pass then leaves the
  // per-utterance sums themselves (nslab = 1: nothing for the excite backward to fold)
  const bool sliced = bn_switches().sliced > 0 && t.dtype == LASR_BF16 && !make_drop(t.dropout).step && C % kSlCh == 0 &&
                      B * (C / kSlCh) >= 128 && T_ >= 64;
  // the BN side of the excite backward (se.hip): fold -> ds -> excite-MLP backward (seg, dW1, dW2) -> BN-backward constants, two launches
  auto excite_bwd = [&](int slabs) {
    SeBwdBn bn;
    bn.partials = partials; bn.nslab = slabs; bn.gamma = m.gamma; bn.beta = m.beta; bn.ysum = se.ysum;
    bn.coef = m.coef; bn.saved = m.saved; bn.coef2 = r.coef; bn.saved2 = r.saved; bn.gamma2 = r.gamma;
    bn.inv_n = 1.0f / (float)(B * T_); bn.tab = tab; bn.dgamma = m.dgamma; bn.dbeta = m.dbeta; bn.dgamma2 = r.dgamma; bn.dbeta2 = r.dbeta;
    return launch_se_bwd(nullptr, &bn, t, se, se_work, st);
  };
  if (sliced) {
    const dim3 grid((unsigned)(C / kSlCh), (unsigned)B);
    with_bool(r.y != nullptr, [&](auto h2) {
      hipLaunchKernelGGL((bn_bwd_stats_sliced_kernel<h2.value, true>), grid, dim3(kSlThreads), 0, st, (const bf16_t*)t.dout, (const bf16_t*)m.y,
                         m.coef, m.saved, (const bf16_t*)r.y, r.coef, r.saved, t.se_scale, partials, (int)(B * T_), (int)C, t.act, (int)T_);
    });
    LASR_LAUNCH_CHECK("bn_bwd_stats_sliced_kernel");
    LASR_TRY(excite_bwd(1));
    // (the apply pass stays on whole-utterance chunks here: the half-utterance form of lasr_bn_act_bwd_apply needs the SE
    //  constants in 128 registers, spills 9 of them and measured 3.80 against 3.78 ms per cfg4 step)
    with_bool(r.y != nullptr, [&](auto h2) {
      hipLaunchKernelGGL((bn_bwd_apply_sliced_kernel<h2.value, true>), grid, dim3(kSlThreads), 0, st, (const bf16_t*)t.dout, (const bf16_t*)m.y,
                         (const bf16_t*)r.y, nullptr, 0, tab, t.se_scale, se.seg, m.coef, m.saved, m.gamma, r.coef, r.saved, r.gamma, 0.f,
                         t.row_lens, (bf16_t*)m.dy, (bf16_t*)r.dy, m.dgamma, m.dbeta, r.dgamma, r.dbeta, (int)(B * T_), (int)T_, (int)C, t.act,
                         (int)T_);
    });
    LASR_LAUNCH_CHECK("bn_bwd_apply_sliced_kernel");
    return 0;
  }
  // pass 1: raw per-(utterance, slab) sums (the SE scale enters the pre-activation z only)
  LASR_TRY(bn_bwd_stats_impl(t, partials, stream, 1));
  LASR_TRY(excite_bwd(nslab));
  // pass 2: dy = G*(d*se + seg) + Bc*y + Cc, dy2 = G2*d + ...
  t.se_grad = se.seg;
  return launch_bn_bwd_apply("lasr_bn_se_bwd", t, tab, st);
}

extern "C" int lasr_bn_eval_coef_many(const lasr_bn_eval_desc* descs, int n_descs, float eps, void* stream) {
  LASR_CHECK_ARG(descs && n_descs >= 1 && n_descs <= 64, "lasr_bn_eval_coef_many: 1..64 layers");
  lasr::BnEvalMany a;
  int64_t cmax = 0;
  for (int i = 0; i < n_descs; ++i) {
    LASR_CHECK_ARG(descs[i].gamma && descs[i].beta && descs[i].running_mean && descs[i].running_var && descs[i].coef && descs[i].C > 0,
                   "lasr_bn_eval_coef_many: bad layer");
    a.d[i] = descs[i];
    cmax = std::max<int64_t>(cmax, descs[i].C);
  }
  hipLaunchKernelGGL(lasr::bn_eval_coef_many_kernel, dim3((unsigned)cdiv(cmax, 256), (unsigned)n_descs), dim3(256), 0, as_stream(stream), a, eps);
  LASR_LAUNCH_CHECK("bn_eval_coef_many_kernel");
  return 0;
}

// ------------------------------------------------------------------ small reductions ----------
namespace lasr {
static constexpr int kColsumRows = 256;
// rows per workgroup: a narrow matrix (the 160-column LSTM gate gradients, the 28-class logit gradient) has only row slabs to make
// workgroups of - 32-row slabs give 501 workgroups at N = 16 032 instead of 63 (24 -> ~6 us for [16 032][160])
static inline int colsum_rows(int64_t C) { return C >= 1024 ? kColsumRows : 32; }
// partials[blk][c] = sum over a 256-row slab.  Narrow matrices (the 28-class logit gradient) would leave most
// of a column-per-thread block idle, so the 256 threads are dealt as col_threads x row_lanes: a lane sums
// every row_lanes-th row of the slab, the lanes are combined through LDS in a fixed order.
// grid (row slabs, column chunks of col_threads): a wide matrix (the 4334-class logit gradient: 444 MB) gets one workgroup per
// (slab, chunk) - 1717 of them - and every thread keeps 8 row loads in flight; with the column loop inside the workgroup
// (101 workgroups, one load in flight per thread) the same sum ran at 0.27 TB/s (1.67 ms per step at cfg5).
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, int64_t rows, int64_t C,
                                                             float* __restrict__ partials, int rows_per_wg) {
  __shared__ float s_p[256];
  const int col_threads = C < 256 ? (int)C : 256;
  const int row_lanes = 256 / col_threads;
  const int cl = threadIdx.x % col_threads, rl = threadIdx.x / col_threads;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
  const int64_t c = (int64_t)blockIdx.y * col_threads + cl;
  float s = 0.f;
  if (rl < row_lanes && c < C) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t r = r0 + rl; r < r1; r += 8 * row_lanes) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t rr = r + (int64_t)u * row_lanes;
        const float xv = x[(rr < r1 ? rr : r1 - 1) * C + c];
        v[u] = rr < r1 ? xv : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += v[u];
    }
    s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  }
  s_p[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0 && c < C) {
    float t = 0.f;
    for (int l = 0; l < row_lanes; ++l) t += s_p[l * col_threads + cl];
    partials[(int64_t)blockIdx.x * C + c] = t;
  }
}
// out[0] = scale * sum(x[0..n)), one wave, fixed order (n is the batch size)
__global__ __launch_bounds__(64) void scale_sum_kernel(const float* __restrict__ x, int64_t n, float scale, float* __restrict__ out) {
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 64) s += x[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[0] = s * scale;
}
// The three small launches behind the dense head's CTC gradient - the row-padded bf16 copy of d(logits) (operand of the decoder's
// two gradient GEMMs), the slab partials of its column sums (decoder bias gradient) and the batch mean of the per-utterance losses
// (train.py:77) - read the same two tensors and do not depend on each other: one grid, three kinds of workgroup (round 4).
__global__ __launch_bounds__(256) void head_tail_kernel(const float* __restrict__ gl, int64_t rows, int64_t C, bf16_t* __restrict__ gl_bf16,
                                                        int64_t ld_out, int n_cast, float* __restrict__ partials, int rows_per_wg, int n_sum,
                                                        const float* __restrict__ nll, int64_t n_nll, float scale, float* __restrict__ loss) {
  const int id = blockIdx.x;
  if (id < n_cast) {                                     // cast_pad_bf16_kernel
    const int64_t total = rows * ld_out;
    for (int64_t i = id * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)n_cast * 256) {
      const int64_t r = i / ld_out, c = i - r * ld_out;
      gl_bf16[i] = c < C ? f32_to_bf16(gl[r * C + c]) : (bf16_t)0;
    }
    return;
  }
  if (id < n_cast + n_sum) {                             // colsum_partial_kernel (C <= 256: one column chunk)
    __shared__ float s_p[256];
    const int blk = id - n_cast;
    const int col_threads = (int)C, row_lanes = 256 / col_threads;
    const int cl = threadIdx.x % col_threads, rl = threadIdx.x / col_threads;
    const int64_t r0 = (int64_t)blk * rows_per_wg;
    const int64_t r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
    float s = 0.f;
    if (rl < row_lanes) {
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int64_t r = r0 + rl; r < r1; r += 8 * row_lanes) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t rr = r + (int64_t)u * row_lanes;
          const float xv = gl[(rr < r1 ? rr : r1 - 1) * C + cl];
          v[u] = rr < r1 ? xv : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] += v[u];
      }
      s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    s_p[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0) {
      float t = 0.f;
      for (int l = 0; l < row_lanes; ++l) t += s_p[l * col_threads + cl];
      partials[(int64_t)blk * C + cl] = t;
    }
    return;
  }
  if (threadIdx.x < 64) {                                // scale_sum_kernel: one wave, fixed order
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n_nll; i += 64) s += nll[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) loss[0] = s * scale;
  }
}
}  // namespace lasr

// the dense small-vocabulary head's tail in one launch (see head_tail_kernel): gl_bf16 = row-padded bf16 copy of gl [rows][C],
// bias_grad = column sums of gl (through `workspace`, second stage = launch_reduce_partials, fixed order), loss = scale * sum(nll).
// Returns 1 (nothing launched) for shapes the merged grid does not take (C > 256).
int lasr::head_tail(const float* gl, int64_t rows, int64_t C, void* gl_bf16, int64_t ld_out, float* bias_grad, void* workspace,
                    size_t workspace_bytes, const float* nll, int64_t n_nll, float scale, float* loss, void* stream) {
  static const bool off = getenv("LASR_HEAD_TAIL_MERGED") && atoi(getenv("LASR_HEAD_TAIL_MERGED")) == 0;
  if (off || C > 256 || C < 1) return 1;
  LASR_CHECK_ARG(gl && gl_bf16 && bias_grad && workspace && nll && loss && rows > 0 && ld_out >= C && n_nll > 0, "head_tail: bad argument");
  if (workspace_bytes < lasr_colsum_workspace_bytes(rows, C)) return fail(LASR_E_WORKSPACE, "head_tail: workspace");
  const int rpw = colsum_rows(C);
  const int n_sum = (int)cdiv(rows, rpw);
  int64_t n_cast = cdiv(rows * ld_out, 256);
  if (n_cast > 256 * 16) n_cast = 256 * 16;
  float* partials = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(lasr::head_tail_kernel, dim3((unsigned)(n_cast + n_sum + 1)), dim3(256), 0, as_stream(stream), gl, rows, C,
                     reinterpret_cast<bf16_t*>(gl_bf16), ld_out, (int)n_cast, partials, rpw, n_sum, nll, n_nll, scale, loss);
  LASR_LAUNCH_CHECK("head_tail_kernel");
  return launch_reduce_partials(partials, n_sum, C, bias_grad, C, nullptr, as_stream(stream));   // f64, fixed order
}

// out[i] = sum_p partials[p*n + i] for up to 64 independent (partials, out, n, n_partials) segments in ONE launch:
// the deferred reductions of a backward stage (split-K slabs of the 1x1 weight gradients, per-(utterance, chunk)
// partials of the depthwise weight gradients).  f64 accumulation in a fixed order, 16 loads in flight.
namespace lasr {
struct ReduceMany { lasr_reduce_desc d[kMaxReduceSegments]; };   // (fused.h)
static constexpr int kReduceEl = 4;        // elements per thread (reduce_many_kernel)
__global__ __launch_bounds__(256) void reduce_many_kernel(ReduceMany a) {
  const lasr_reduce_desc& q = a.d[blockIdx.y];
  const int64_t i0 = (int64_t)blockIdx.x * (256 * kReduceEl) + threadIdx.x;
  if (q.n_partials <= 4 && i0 >= q.n) return;
  if (q.n_partials <= 4 && i0 + 256 * (kReduceEl - 1) < q.n) {
    // split-K slabs (2-4 partials): kReduceEl elements per thread with all of their loads in flight before the first add (one
    // element per thread left 3 loads in flight per lane: 59 MB at 2 TB/s).  Per element the same f64 sum in the same order as
    // reduce_many_elem (partials 0..3 into accumulators a0..a3, then (a0 + a1) + (a2 + a3)).
    float v[kReduceEl][4];
#pragma unroll
    for (int e = 0; e < kReduceEl; ++e)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float x = q.partials[(int64_t)min(u, q.n_partials - 1) * q.n + i0 + 256 * e];
        v[e][u] = u < q.n_partials ? x : 0.f;
      }
#pragma unroll
    for (int e = 0; e < kReduceEl; ++e) {
      const double a0 = 0.0 + (double)v[e][0], a1 = 0.0 + (double)v[e][1], a2 = 0.0 + (double)v[e][2], a3 = 0.0 + (double)v[e][3];
      q.out[i0 + 256 * e] = (float)((a0 + a1) + (a2 + a3));
    }
    return;
  }
  if (q.n_partials <= 4) {                                 // a slab segment's ragged last block
#pragma unroll 1
    for (int e = 0; e < kReduceEl; ++e) {
      const int64_t i = i0 + 256 * e;
      if (i < q.n) reduce_many_elem(q, i);                 // reduce_body.h
    }
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // many partials: one element per thread, 16 loads in flight each
  if (i < q.n) reduce_many_elem(q, i);
}
}  // namespace lasr

extern "C" int lasr_reduce_many(const lasr_reduce_desc* descs, int n_descs, void* stream) {
  LASR_CHECK_ARG(descs && n_descs >= 1 && n_descs <= lasr::kMaxReduceSegments, "lasr_reduce_many: 1..%d segments", lasr::kMaxReduceSegments);
  lasr::ReduceMany a;
  int64_t nmax = 0;
  static const bool dump = getenv("LASR_REDUCE_DUMP") != nullptr;      // dev aid: the segments of every launch on stderr
  if (dump) {
    fprintf(stderr, "lasr_reduce_many: %d segments:", n_descs);
    for (int i = 0; i < n_descs; ++i) fprintf(stderr, " %lldx%d", (long long)descs[i].n, descs[i].n_partials);
    fprintf(stderr, "\n");
  }
  for (int i = 0; i < n_descs; ++i) {
    LASR_CHECK_ARG(descs[i].partials && descs[i].out && descs[i].n > 0 && descs[i].n_partials > 0, "lasr_reduce_many: bad segment");
    a.d[i] = descs[i];
    nmax = std::max<int64_t>(nmax, cdiv(descs[i].n, descs[i].n_partials <= 4 ? 256 * lasr::kReduceEl : 256));   // blocks this segment needs
  }
  hipLaunchKernelGGL(lasr::reduce_many_kernel, dim3((unsigned)nmax, (unsigned)n_descs), dim3(256), 0, as_stream(stream), a);
  LASR_LAUNCH_CHECK("reduce_many_kernel");
  return 0;
}

extern "C" size_t lasr_colsum_workspace_bytes(int64_t rows, int64_t C) {
  return (size_t)cdiv(rows, colsum_rows(C)) * C * sizeof(float);
}
extern "C" int lasr_colsum_f32(const float* x, float* out, int64_t rows, int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
  LASR_CHECK_ARG(x && out && workspace && rows > 0 && C > 0, "lasr_colsum_f32: bad argument");
  if (workspace_bytes < lasr_colsum_workspace_bytes(rows, C)) return fail(LASR_E_WORKSPACE, "lasr_colsum_f32: workspace");
  const int rpw = colsum_rows(C);
  const int nblk = (int)cdiv(rows, rpw);
  float* partials = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(nblk, (unsigned)cdiv(C, C < 256 ? C : 256)), dim3(256), 0, as_stream(stream), x, rows, C, partials, rpw);
  LASR_LAUNCH_CHECK("colsum_partial_kernel");
  return launch_reduce_partials(partials, nblk, C, out, C, nullptr, as_stream(stream));   // f64, fixed order
}
extern "C" int lasr_scale_sum_f32(const float* x, int64_t n, float scale, float* out, void* stream) {
  LASR_CHECK_ARG(x && out && n > 0, "lasr_scale_sum_f32: bad argument");
  hipLaunchKernelGGL(scale_sum_kernel, dim3(1), dim3(64), 0, as_stream(stream), x, n, scale, out);
  LASR_LAUNCH_CHECK("scale_sum_kernel");
  return 0;
}
