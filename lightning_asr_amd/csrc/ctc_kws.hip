// CTC keyword search: the third member of the lattice family of ctc_lattice.h - a max-product walk like forced alignment's
// (ctc_align.hip), with a free start and a free end, over the 2L-1 states of a phrase (no leading or trailing blank), on
// filler-normalised emissions e_t(j) = logp[t][cls(j)] - max_c logp[t][c].  Every state carries (v, s): the score and the frame
// its path entered state 0; the end state's (E_t, S_t) is the trace the hits are picked from, in the same launch.
// Definition: include/lasr.h, lasr_ctc_kws.
//
// One wave owns one (utterance, keyword) pair; a workgroup is kKwsWaves waves on kKwsWaves consecutive keywords of ONE
// utterance, the grid runs over (utterance, keyword group): with B = 1 the parallelism comes from K.
// States: one per lane for L <= 32 (2L-1 <= 63), two per lane above (lane i: label i and the blank after it; L <= 64), chosen
// per wave.  Both v and s move to the neighbour lanes by DPP shifts; no LDS round trip on the dependent chain.
// Emissions: EM_LDS - the utterance's rows staged once per workgroup (ctc_fill_emissions) and the exact row maxima taken from
// the staged rows, all waves share both, the next frame's values are read before this frame's arithmetic; otherwise each lane
// gathers its class's value, and the row maximum a pre-pass left in the workspace, a chunk of kKwsPre frames ahead: the
// addresses do not depend on the recursion, so no step of the chain waits on a load.
// Picking runs inline on every lane over its own (garbage but harmless) trace; only the lane of the end state stores.  Starts
// are outputs only, never an index.
#include "ctc_lattice.h"

namespace lasr {

static constexpr int kKwsWaves = 8;                 // keywords (waves) per workgroup: they share one staged copy of the rows
static constexpr int kKwsThreads = 64 * kKwsWaves;
static constexpr int kKwsPre = 8;                   // frames per chunk of the global gather, fetched one chunk ahead
static constexpr int kKwsNoStart = 0x7fffffff;      // the start of a dead state: loses every tie

__host__ __device__ static inline size_t kws_max_bytes(int64_t T) { return ((size_t)T * sizeof(float) + 15) / 16 * 16; }

__device__ __forceinline__ int wave_shr1_i(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); }

struct KwsCell {
  float v;
  int s;
};
// a, unless b is better: the larger v, on equal v the smaller s.  Bitwise on purpose (as in KwsPicker::frame): `||` and `&&`
// compiled to an exec-mask branch per operator, ten s_and_saveexec regions on the dependent chain of every frame.
__device__ __forceinline__ KwsCell kws_better(KwsCell a, KwsCell b) {
  const bool take = (b.v > a.v) | ((b.v == a.v) & (b.s < a.s));
  KwsCell r;
  r.v = take ? b.v : a.v;
  r.s = take ? b.s : a.s;
  return r;
}
// every lane the cell of the lane below; lane 0 gets `fill`
__device__ __forceinline__ KwsCell kws_shr1(KwsCell a, float fill_v, int fill_s) {
  KwsCell r;
  r.v = wave_shr1(a.v, fill_v);
  r.s = wave_shr1_i(a.s, fill_s);
  return r;
}

// The hits and the best frame of one pair, fed the end trace frame by frame.  Every lane runs it; `own` (the lane of the end
// state) alone stores.
struct KwsPicker {
  float thr;
  int max_hits;
  bool own;
  int32_t* __restrict__ span;     // this pair's (max_hits, 2)
  float* __restrict__ score;      // this pair's (max_hits)
  bool pending = false;
  int p_s = 0, p_e = 0, n = 0;
  float p_v = 0.f;
  float best = kNegInf;
  int b_s = -1, b_e = -1;
  __device__ __forceinline__ void emit() {
    if (own & (n < max_hits)) {
      span[2 * n] = p_s;
      span[2 * n + 1] = p_e;
      score[n] = p_v;
    }
    ++n;
  }
  // branch-free but for the store of a hit that leaves
  __device__ __forceinline__ void frame(int t, float E, int S) {
    const bool nb = (E > 0.5f * kDead) & (E >= best);     // live; the latest frame wins ties
    best = nb ? E : best;
    b_s = nb ? S : b_s;
    b_e = nb ? t + 1 : b_e;
    const bool cand = E >= thr;
    const bool overlap = pending & (S < p_e);
    const bool leave = cand & pending & !overlap;
    if (leave & own & (n < max_hits)) {
      span[2 * n] = p_s;
      span[2 * n + 1] = p_e;
      score[n] = p_v;
    }
    n += leave ? 1 : 0;
    const bool take = cand & (!overlap | (E >= p_v));     // the later candidate wins ties
    p_s = take ? S : p_s;
    p_e = take ? t + 1 : p_e;
    p_v = take ? E : p_v;
    pending |= cand;
  }
};

// The walk of one wave over its pair: NS = 1 - lane j holds state j; NS = 2 - lane i holds states 2i (label i) and 2i+1 (the
// blank after it).  The end state is a[0] of lane 2L-2 / L-1.  States past 2L-2 never feed a lower one and are never read.
// rows: EM_LDS - the staged rows, row t at rows + t * C with a pad row after the last; else the utterance's logp.
// rmax: the row maxima of the utterance (LDS / workspace).
template <int NS, bool EM_LDS>
__device__ __forceinline__ void kws_walk(const float* rows, const float* rmax, const int32_t* __restrict__ lab, int L, int Tb, int C,
                                         int blank, int lane, KwsPicker& pk) {
  const int li = min(NS == 1 ? lane >> 1 : lane, L - 1);            // the label this lane's a[0] stands for (clamped: unused lanes)
  const int mine = min(max(lab[li], 0), C - 1);
  const int prev = min(max(lab[max(li - 1, 0)], 0), C - 1);
  const bool is_label = NS == 2 || !(lane & 1);
  const bool skip_ok = is_label && li >= 1 && mine != prev;
  int cls[NS];
  cls[0] = is_label ? mine : blank;
  if (NS == 2) cls[NS - 1] = blank;
  pk.own = lane == (NS == 1 ? 2 * L - 2 : L - 1);
  KwsCell a[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    a[i].v = kDead;
    a[i].s = kKwsNoStart;
  }
  // one frame: a[] (t-1) -> a[] (t) with the raw emissions em[] and the row maximum m.  The fresh start (0, t) of state 0 is the
  // fill lane 0 receives as its "state -1"; a skip that does not exist is a dead candidate.  No branch.
  auto step = [&](int t, const float (&em)[NS], float m) {
    const KwsCell p1 = kws_shr1(a[NS - 1], 0.f, t);                 // state j-1 (NS = 2: the blank before this label)
    KwsCell p2 = NS == 1 ? kws_shr1(p1, kDead, kKwsNoStart) : kws_shr1(a[0], kDead, kKwsNoStart);   // state j-2
    p2.v = skip_ok ? p2.v : kDead;
    const KwsCell c0 = kws_better(kws_better(a[0], p1), p2);
    if (NS == 2) {
      const KwsCell c1 = kws_better(a[NS - 1], a[0]);
      a[NS - 1].v = c1.v + (em[NS - 1] - m);
      a[NS - 1].s = c1.s;
    }
    a[0].v = c0.v + (em[0] - m);
    a[0].s = c0.s;
    pk.frame(t, a[0].v, a[0].s);
  };
  if (Tb <= 0) return;
  float em[NS];
  if (EM_LDS) {
    float nx[NS], nm = rmax[0];
#pragma unroll
    for (int i = 0; i < NS; ++i) nx[i] = rows[cls[i]];
    const float* row = rows;
    for (int t = 0; t < Tb; ++t) {
      const float m = nm;
#pragma unroll
      for (int i = 0; i < NS; ++i) em[i] = nx[i];
      row += C;                                                     // the next frame's values: issued before this frame's arithmetic
      nm = rmax[min(t + 1, Tb - 1)];                                // (the last one reads the pad row)
#pragma unroll
      for (int i = 0; i < NS; ++i) nx[i] = row[cls[i]];
      step(t, em, m);
    }
  } else {
    // Chunks of kKwsPre frames in two register buffers, one chunk ahead of the walk (the backtrace of ctc_align.hip fetches its
    // rows the same way): the loads of a chunk are issued before the first frame of the chunk before it and first used kKwsPre
    // frames later, and the buffers swap roles in the twice-unrolled loop, so nothing is copied.  A register ring refilled frame
    // by frame waited for ALL its loads once per round: s_waitcnt vmcnt counts the conditional stores of the hits too, and
    // across the loop's back edge the compiler asked for vmcnt(0).
    float bufa[kKwsPre][NS], bufb[kKwsPre][NS], ma[kKwsPre], mb[kKwsPre];
    auto fetch = [&](float (&w)[kKwsPre][NS], float (&wm)[kKwsPre], int t_lo) {
#pragma unroll
      for (int u = 0; u < kKwsPre; ++u) {
        const int tq = min(t_lo + u, Tb - 1);                       // a clamped row is fetched and not used
#pragma unroll
        for (int i = 0; i < NS; ++i) w[u][i] = rows[(int64_t)tq * C + cls[i]];
        wm[u] = rmax[tq];
      }
    };
    auto walk = [&](const float (&w)[kKwsPre][NS], const float (&wm)[kKwsPre], int t_lo) {
#pragma unroll
      for (int u = 0; u < kKwsPre; ++u) {
        const int t = t_lo + u;
        if (t < Tb) {                                               // wave-uniform
#pragma unroll
          for (int i = 0; i < NS; ++i) em[i] = w[u][i];
          step(t, em, wm[u]);
        }
      }
    };
    fetch(bufa, ma, 0);
    for (int t0 = 0; t0 < Tb; t0 += 2 * kKwsPre) {
      fetch(bufb, mb, t0 + kKwsPre);
      walk(bufa, ma, t0);
      fetch(bufa, ma, t0 + 2 * kKwsPre);
      walk(bufb, mb, t0 + kKwsPre);
    }
  }
}

// Row maxima of logp (rows x C) for the global-gather form: one wave per row, the exact maximum (a max does not round).
__global__ __launch_bounds__(kKwsThreads) void ctc_kws_rowmax_kernel(const float* __restrict__ logp, int64_t rows, int64_t C,
                                                                      float* __restrict__ rmax) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kKwsWaves + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* p = logp + r * C;
  float m = kNegInf;
  for (int64_t c = lane; c < C; c += 64) m = fmaxf(m, p[c]);
  m = wave_max(m);
  if (lane == 0) rmax[r] = m;
}

template <bool EM_LDS>
__global__ __launch_bounds__(kKwsThreads) void ctc_kws_kernel(const float* __restrict__ logp, const int32_t* __restrict__ in_lens, int64_t T,
                                                               int64_t C, int blank, const int32_t* __restrict__ kw_labels,
                                                               const int32_t* __restrict__ kw_offsets, int64_t K, int groups, int L_max,
                                                               float threshold, int max_hits, int32_t* __restrict__ n_hits,
                                                               int32_t* __restrict__ hit_span, float* __restrict__ hit_score,
                                                               float* __restrict__ best_score, int32_t* __restrict__ best_span,
                                                               const float* __restrict__ rmax_ws) {
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  const int b = (int)(blockIdx.x / (unsigned)groups);
  const int g = (int)(blockIdx.x % (unsigned)groups);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int Tb = in_lens ? min(max(in_lens[b], 0), (int)T) : (int)T;
  const float* lp = logp + (int64_t)b * T * C;
  // dynamic LDS (EM_LDS): [emission block (T + 2) x C] [row maxima, T]
  float* s_lp = s_dyn;
  float* s_max = reinterpret_cast<float*>(reinterpret_cast<char*>(s_dyn) + ctc_em_bytes(T, C));
  if (EM_LDS) {
    if (Tb > 0) ctc_fill_emissions(lp, Tb, C, kKwsThreads, s_lp);
    __syncthreads();
    for (int t = threadIdx.x; t < Tb; t += kKwsThreads) {
      const float* row = s_lp + (int64_t)(t + 1) * C;
      float m = kNegInf;
      for (int c = 0; c < (int)C; ++c) m = fmaxf(m, row[c]);
      s_max[t] = m;
    }
    __syncthreads();
  }
  const int64_t k = (int64_t)g * kKwsWaves + wv;
  if (k >= K) return;                                               // wave-uniform; no barrier below

  const int total = kw_offsets[K];
  const int off = kw_offsets[k];
  const int base = min(max(off, 0), max(total - 1, 0));
  const int L = min(max(kw_offsets[k + 1] - off, 1), min(L_max, max(total - base, 1)));
  const int64_t pair = (int64_t)b * K + k;
  KwsPicker pk;
  pk.thr = threshold * (float)L;
  pk.max_hits = max_hits;
  pk.own = false;
  pk.span = hit_span + pair * max_hits * 2;
  pk.score = hit_score + pair * max_hits;
  const float* rows = EM_LDS ? s_lp + C : lp;
  const float* rmax = EM_LDS ? s_max : rmax_ws + (int64_t)b * T;
  if (L <= 32) kws_walk<1, EM_LDS>(rows, rmax, kw_labels + base, L, Tb, (int)C, blank, lane, pk);
  else kws_walk<2, EM_LDS>(rows, rmax, kw_labels + base, L, Tb, (int)C, blank, lane, pk);
  if (pk.pending) pk.emit();
  if (pk.own) {
    n_hits[pair] = pk.n;
    best_score[pair] = pk.best;
    best_span[2 * pair] = pk.b_s;
    best_span[2 * pair + 1] = pk.b_e;
  }
  // the slots no hit reached: (-1, -1) and 0, by all lanes
  const int end_lane = L <= 32 ? 2 * L - 2 : L - 1;
  const int n = __builtin_amdgcn_readlane(pk.n, __builtin_amdgcn_readfirstlane(end_lane));
  for (int i = min(n, max_hits) + lane; i < max_hits; i += 64) {
    pk.span[2 * i] = -1;
    pk.span[2 * i + 1] = -1;
    pk.score[i] = 0.f;
  }
}

}  // namespace lasr

using namespace lasr;

extern "C" size_t lasr_ctc_kws_workspace_bytes(int64_t B, int64_t T, int64_t K) {
  if (B <= 0 || T <= 0 || K <= 0) return 0;
  return align_up((size_t)B * T * sizeof(float), 256);              // the row maxima of the global-gather form
}

extern "C" int lasr_ctc_kws(const float* logp, const int32_t* in_lens, int64_t B, int64_t T, int64_t C, int blank, const int32_t* kw_labels,
                            const int32_t* kw_offsets, int64_t K, int64_t L_max, float threshold, int max_hits, int32_t* n_hits,
                            int32_t* hit_span, float* hit_score, float* best_score, int32_t* best_span, void* workspace,
                            size_t workspace_bytes, void* stream) {
  LASR_CHECK_ARG(logp && kw_labels && kw_offsets && n_hits && hit_span && hit_score && best_score && best_span && workspace,
                 "lasr_ctc_kws: null pointer");
  LASR_CHECK_SHAPE(L_max >= 1 && L_max <= LASR_KWS_MAX_LABELS, "lasr_ctc_kws: L_max=%lld outside [1, %d], the label bound of a keyword",
                   (long long)L_max, LASR_KWS_MAX_LABELS);
  LASR_CHECK_SHAPE(B > 0 && T > 0 && C > 1 && K >= 1 && max_hits >= 1 && blank >= 0 && blank < C && T * C < (int64_t)1 << 31,
                   "lasr_ctc_kws: shape");
  const int64_t groups = cdiv(K, kKwsWaves);
  LASR_CHECK_SHAPE(B * groups < (int64_t)1 << 31 && B * K * max_hits < (int64_t)1 << 31, "lasr_ctc_kws: shape (B * K)");
  LASR_CHECK_ARG(threshold > -1e6f && threshold <= 0.f, "lasr_ctc_kws: threshold %g outside (-1e6, 0]", (double)threshold);
  if (workspace_bytes < lasr_ctc_kws_workspace_bytes(B, T, K)) return fail(LASR_E_WORKSPACE, "lasr_ctc_kws: workspace");
  // LDS budget: the row maxima beside the emission block, when that fits (ctc_em_in_lds)
  const bool em_lds = ctc_em_in_lds(T, C, kCtcLdsHeadroom + kws_max_bytes(T), logp);
  const size_t lds = em_lds ? ctc_em_bytes(T, C) + kws_max_bytes(T) : 0;
  hipStream_t st = as_stream(stream);
  float* rmax = static_cast<float*>(workspace);
  if (!em_lds) {
    hipLaunchKernelGGL(ctc_kws_rowmax_kernel, dim3((unsigned)cdiv(B * T, kKwsWaves)), dim3(kKwsThreads), 0, st, logp, B * T, C, rmax);
    LASR_LAUNCH_CHECK("ctc_kws_rowmax_kernel");
  }
  with_bool(em_lds, [&](auto em) {
    launch_lds(ctc_kws_kernel<decltype(em)::value>, dim3((unsigned)(B * groups)), dim3(kKwsThreads), lds, st, logp, in_lens, T, C, blank,
               kw_labels, kw_offsets, K, (int)groups, (int)L_max, threshold, max_hits, n_hits, hit_span, hit_score, best_score, best_span,
               static_cast<const float*>(rmax));
  });
  LASR_LAUNCH_CHECK("ctc_kws_kernel");
  return 0;
}
