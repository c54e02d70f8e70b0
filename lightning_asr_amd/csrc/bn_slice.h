// GEMM-epilogue BatchNorm partial sums -> training-mode BN coefficients, as device functions: the stand-alone finalize launches
// (norm.hip) and the consumer-side finalize of a 64-channel slice in the prologue of the kernels that apply a unit's BatchNorm
// (bn_act_fwd_sliced_kernel in norm.hip, dwconv_s1_mfma_bn_kernel in conv.hip) run the same arithmetic in the same order.
#pragma once
#include "common.h"

namespace lasr {

__device__ __forceinline__ void bn_finalize_channel(float s, float q, int64_t c, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ rmean,
                                                    float* __restrict__ rvar, float* __restrict__ coef, float* __restrict__ saved,
                                                    int64_t C, float n, float eps, float momentum, int training) {
  float mean, var;
  if (training) {
    // sums arrive in f32; the subtraction is done in double to keep E[x^2]-E[x]^2 benign
    // (Which products fuse with the add that follows is written out, not left to the compiler: inlined into different kernels it chose
    //  differently - fused here, two rounded products there - and the kernels that share this function must give the same bits.  The
    //  forms below are the ones every finalize kernel of the library has always been compiled to.)
    const double m = (double)s / n;
    double v = fma(-m, m, (double)q / n);
    if (v < 0) v = 0;
    mean = (float)m;
    var = (float)v;
    if (rmean) {
#pragma clang fp contract(off)
      const float keep = 1.f - momentum;
      const float km = keep * rmean[c], nm = momentum * mean;
      rmean[c] = km + nm;
      const float unbiased = n > 1.f ? (float)(v * (double)n / ((double)n - 1.0)) : var;
      const float kv = keep * rvar[c], nv = momentum * unbiased;
      rvar[c] = kv + nv;
    }
  } else {
    mean = rmean[c];
    var = rvar[c];
  }
  const float rstd = 1.0f / sqrtf(var + eps);
  const float a = gamma[c] * rstd;
  coef[c] = a;
  coef[C + c] = fmaf(-a, mean, beta[c]);
  if (saved) { saved[c] = mean; saved[C + c] = rstd; }
}

// ------------------------------------------------------------------ fixed-order partial sums ----
// block = 32 columns x 8 partial lanes; each lane strides the partial rows with 4 independent sums.
// Accumulation is f64: these sums are BatchNorm statistics and gradient reductions, and the
// network's backward map amplifies relative noise in them by ~1e2-1e3 (measured), so f32 sums
// of a few hundred partials cost visible gradient parity.
// one partial lane's share of column c: rows pl, pl+8, ... in a fixed order.  The partials were written by the
// previous kernel on other XCDs, so every load is a trip to the fabric: 16 rows are requested before the
// first is added (a loop of 4 loads per trip exposed that latency ~16 times for 501 rows: 8.6 us per call).
template <int LANES = 8>
__device__ __forceinline__ double partial_lane_sum(const float* __restrict__ partials, int n_part, int64_t ncols, int64_t c, int pl) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int p = pl; p < n_part; p += 16 * LANES) {
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = p + LANES * i;
      const float x = partials[(int64_t)min(r, n_part - 1) * ncols + c];   // clamped address, masked value: no branch around the load
      v[i] = r < n_part ? x : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
      a0 += (double)v[i]; a1 += (double)v[i + 1]; a2 += (double)v[i + 2]; a3 += (double)v[i + 3];
    }
  }
  return (a0 + a1) + (a2 + a3);
}

// partial_lane_sum (8 lanes) of NC columns that share n_part and the row pitch, per column the same adds in the same order - but the
// 16 x NC loads of a batch are all requested before the first add, so a thread that owns several columns pays one round trip per
// batch, not one per column.
template <int NC>
__device__ __forceinline__ void partial_lane_sum_cols(const float* const (&col)[NC], int n_part, int64_t ncols, int pl, double (&out)[NC]) {
  double a[NC][4];
#pragma unroll
  for (int k = 0; k < NC; ++k) a[k][0] = a[k][1] = a[k][2] = a[k][3] = 0.0;
  for (int p = pl; p < n_part; p += 16 * 8) {
    float v[NC][16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = p + 8 * i;
      const int64_t ro = (int64_t)min(r, n_part - 1) * ncols;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const float x = col[k][ro];
        v[k][i] = r < n_part ? x : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k)
#pragma unroll
      for (int i = 0; i < 16; i += 4) {
        a[k][0] += (double)v[k][i]; a[k][1] += (double)v[k][i + 1]; a[k][2] += (double)v[k][i + 2]; a[k][3] += (double)v[k][i + 3];
      }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) out[k] = (a[k][0] + a[k][1]) + (a[k][2] + a[k][3]);
}

struct BnBranch {
  const float* partials; int n_part;
  const float* gamma; const float* beta; float* rmean; float* rvar; float* coef; float* saved; float* stats;
};
struct BnBranch2 { BnBranch b[2]; };

// A unit's BatchNorm finalize left to the kernel that applies it (the forward's "statistics -> apply, nothing in between"):
// what the consumer needs besides the branches.  nb = 0: the coefficients are in memory already (the separate finalize launch ran).
struct BnSliceIn { BnBranch2 br; int nb; float n, eps, momentum; };

static constexpr int kBnSliceCh = 64;                       // channels of a slice
static constexpr int kBnSliceAccBytes = 8 * 4 * kBnSliceCh * 8;   // s_acc: [8 partial lanes][2 branches x (sum | sumsq)][64] f64
static constexpr int kBnSliceTabFloats = 2 * 4 * kBnSliceCh;      // s_tab: [2 branches][a | b | mean | rstd][64] f32

// The coefficients of channels [c0, c0 + 64) of one or two branches from their partials ([n_part][sum | sumsq][C]), by a workgroup of
// 512 threads: bn_finalize_partials_kernel's arithmetic - lane pl of 8 sums partials pl, pl + 8, ... (partial_lane_sum), the 8 lane sums
// are added in order in f64, both sums are cast to f32, then bn_finalize_channel - so the numbers are that launch's numbers.
// Every global load (the thread's partials; gamma, beta and the running statistics of the finalizing threads) is requested before
// the first add.  The slice's a | b | mean | rstd land in s_tab; `writer` (exactly one workgroup per slice) also leaves coef, saved,
// stats and the running statistics in memory, where the backward, the taps and eval read them.  Two barriers inside; the caller
// reads s_tab behind the second.  No wait on any other workgroup.
template <bool HAS2>
__device__ __forceinline__ void bn_slice_finalize(const BnSliceIn& in, int C, int c0, bool writer, double* __restrict__ s_acc,
                                                  float* __restrict__ s_tab) {
  constexpr int NB = HAS2 ? 2 : 1;
  const int tid = threadIdx.x, ch = tid & 63, pl = tid >> 6;
  const BnBranch& b0 = in.br.b[0];
  const BnBranch& b1 = in.br.b[1];
  // the finalizing threads' per-channel inputs: waves 0 (main) and 1 (residual), requested with the partials
  // (every thread loads them, from a valid address whatever the branch carries: no branch around a load; the branch's pointers are
  //  picked one by one with a wave-uniform condition - a reference to the picked struct would copy it to scratch)
  const bool fin = tid < NB * kBnSliceCh;
  const bool second = HAS2 && __builtin_amdgcn_readfirstlane(pl) == 1;
  const int cf = c0 + ch;
  const float* gp = second ? b1.gamma : b0.gamma;
  const float* bp = second ? b1.beta : b0.beta;
  float* rmean = second ? b1.rmean : b0.rmean;
  float* rvar = second ? b1.rvar : b0.rvar;
  float* coef = second ? b1.coef : b0.coef;
  float* saved = second ? b1.saved : b0.saved;
  float* stats = second ? b1.stats : b0.stats;
  float g = gp[cf], be = bp[cf], rm = (rmean ? rmean : gp)[cf], rv = (rmean ? rvar : gp)[cf];
  const int64_t nc = 2 * (int64_t)C;
  if (HAS2 && b0.n_part == b1.n_part) {                    // workgroup-uniform (the model's units: both branches share the row tiling)
    const float* const col[4] = {b0.partials + cf, b0.partials + C + cf, b1.partials + cf, b1.partials + C + cf};
    double o[4];
    partial_lane_sum_cols<4>(col, b0.n_part, nc, pl, o);
#pragma unroll
    for (int k = 0; k < 4; ++k) s_acc[(pl * 4 + k) * kBnSliceCh + ch] = o[k];
  } else {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const BnBranch& b = j ? b1 : b0;
      const float* const col[2] = {b.partials + cf, b.partials + C + cf};
      double o[2];
      partial_lane_sum_cols<2>(col, b.n_part, nc, pl, o);
      s_acc[(pl * 4 + 2 * j) * kBnSliceCh + ch] = o[0];
      s_acc[(pl * 4 + 2 * j + 1) * kBnSliceCh + ch] = o[1];
    }
  }
  __syncthreads();
  if (fin) {
    const int j = pl;                                      // branch
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { s += s_acc[(i * 4 + 2 * j) * kBnSliceCh + ch]; q += s_acc[(i * 4 + 2 * j + 1) * kBnSliceCh + ch]; }
    float* tab = s_tab + j * 4 * kBnSliceCh;               // [a | b][64], then [mean | rstd][64]
    const bool upd = writer && rmean;
    bn_finalize_channel((float)s, (float)q, 0, &g, &be, upd ? &rm : nullptr, upd ? &rv : nullptr, tab + ch, tab + 2 * kBnSliceCh + ch,
                        kBnSliceCh, in.n, in.eps, in.momentum, 1);
    if (writer) {
      if (stats) { stats[cf] = (float)s; stats[C + cf] = (float)q; }
      if (upd) { rmean[cf] = rm; rvar[cf] = rv; }
      coef[cf] = tab[ch]; coef[C + cf] = tab[kBnSliceCh + ch];
      if (saved) { saved[cf] = tab[2 * kBnSliceCh + ch]; saved[C + cf] = tab[3 * kBnSliceCh + ch]; }
    }
  }
  __syncthreads();
}

}  // namespace lasr
