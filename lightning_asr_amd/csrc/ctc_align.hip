// CTC forced alignment: the max-product (Viterbi) member of the lattice family of ctc_lattice.h, with its backtrace and the
// per-label spans, in one launch.  The walk is the one of the loss's sum-product recursion (ctc_lattice.h: label and emission
// staging, the state table, the emission stream, the edge exchange); this file keeps the per-state operator (max + backpointer
// with its tie rule), the packed backpointer table, the backtrace and the span pass.
//
// Definition (include/lasr.h, lasr_ctc_align): v[0][s] = logp[0][cls(s)] for s in {0, 1}; v[t][s] = max(stay, step, skip) +
// logp[t][cls(s)] in f32, one rounding per state per frame; the backpointer is the candidate that attains the max, on equality
// stay before step before skip; the path ends in state 2S when v[2S] >= v[2S-1] (or S = 0), else in 2S-1.
//
// One workgroup per utterance.  S_max <= 511: wave 0 holds the 2S+1 states 4 / 8 / 16 per lane and runs the recursion alone,
// three helper waves take part in the LDS fill and the span pass.  Longer labels: 2..4 waves of 16 states per lane, edge states
// through the two-slot LDS ring of CtcEdge (one lds_barrier per step).
// Backpointers: 2 bits per state, so the NS <= 16 states of a lane are ONE dword per lane per frame: a row is 64 dwords per
// wave (256 B where the loss lattice stores 64 * NS * 4).  The table lives in LDS when it fits beside the emission block and the
// label table, in the workspace otherwise.
// Backtrace: wave 0 walks frames Tb-1 .. 1 with the state in a scalar register.  A row's address does not depend on the state
// (only which lane's dword is wanted does), so rows are fetched 16 at a time, one chunk ahead of the walk, each lane its own
// dword; the dependent chain per frame is v_readlane + shift + subtract.  The state is clamped to >= 0 and only ever
// decreases from <= 2S, so whatever the table holds (NaN emissions make every compare false) the walk stays in the lattice.
#include "ctc_lattice.h"

namespace lasr {

static constexpr int kAlignThreads = 256;   // one-wave form: wave 0 + three helper waves
static constexpr int kAlignBtRows = 16;     // backpointer rows per backtrace chunk

// bytes of one utterance's backpointer table / of the frame-state row a workgroup keeps in LDS
static inline size_t align_bp_bytes(int64_t T, int nw) { return (size_t)T * 64 * nw * sizeof(uint32_t); }
__host__ __device__ static inline size_t align_state_bytes(int64_t T) { return ((size_t)T * sizeof(int32_t) + 15) / 16 * 16; }

template <int NS, bool MW, bool EM_LDS, bool BP_LDS>
__global__ __launch_bounds__(256) void ctc_align_kernel(const float* __restrict__ logp, const int64_t* __restrict__ targets,
                                                        const int32_t* __restrict__ in_lens, const int32_t* __restrict__ tgt_lens,
                                                        int64_t T, int64_t C, int64_t S_max, int blank, float* __restrict__ score,
                                                        int32_t* __restrict__ frame_state, float* __restrict__ frame_logp,
                                                        int32_t* __restrict__ label_start, int32_t* __restrict__ label_end,
                                                        uint32_t* __restrict__ bp_ws) {
  static_assert(!MW || NS == kCtcMwNS, "the multi-wave form holds 16 states per lane");
  constexpr int LOG_NS = NS == 4 ? 2 : (NS == 8 ? 3 : 4);
  constexpr int NWR = MW ? kCtcMwMaxWaves : 1;      // dwords per lane of one backpointer row in the backtrace
  __shared__ int32_t s_tg[kCtcMwMaxS];
  __shared__ float s_ring[kCtcRingFloats];
  __shared__ float s_fin[2];
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  const int NT = (int)blockDim.x;
  const int NW = MW ? NT >> 6 : 1;
  const int RW = 64 * NW;                            // dwords per backpointer row
  const int b = (int)blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int Tb = in_lens ? min(max(in_lens[b], 0), (int)T) : (int)T;
  const int S = min(max(tgt_lens[b], 0), (int)S_max);
  const int SS = 2 * S + 1;
  const float* lp = logp + (int64_t)b * T * C;
  // dynamic LDS: [emission block (T + 2) x C] [frame states, T] [backpointer table T x RW]
  float* s_lp = s_dyn;
  int32_t* s_st = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(s_dyn) + (EM_LDS ? ctc_em_bytes(T, C) : 0));
  uint32_t* s_bp = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(s_st) + align_state_bytes(T));
  uint32_t* g_bp = bp_ws + (int64_t)b * T * RW;

  ctc_load_labels(targets + (int64_t)b * S_max, S, C - 1, NT, s_tg);
  for (int i = threadIdx.x; i < (int)S_max; i += NT) {   // spans of labels the path does not open stay -1
    label_start[(int64_t)b * S_max + i] = -1;
    label_end[(int64_t)b * S_max + i] = -1;
  }
  ctc_edge_init(s_ring, s_fin);                         // s_fin: v[Tb-1][2S-1], v[Tb-1][2S]
  if (EM_LDS && Tb > 0) ctc_fill_emissions(lp, Tb, C, NT, s_lp);
  __syncthreads();
  if (Tb <= 0) {                                       // workgroup-uniform: no frame, so no path unless there is no label either
    if (threadIdx.x == 0) score[b] = (S == 0) ? 0.f : kNegInf;
    for (int t = threadIdx.x; t < (int)T; t += NT) {
      frame_state[(int64_t)b * T + t] = -1;
      frame_logp[(int64_t)b * T + t] = 0.f;
    }
    return;
  }

  // ------------------------------------------------------------------ recursion
  if (wv < NW) {
    const int s0 = wv * (64 * NS) + lane * NS;          // this lane's first state
    int cls4[NS];
    bool skip_ok[NS];
    float a[NS];
    LASR_CTC_LATTICE_STATES(NS, false, false, s_tg, s0, SS, blank, lp, cls4, skip_ok, a)
    CtcEdge<MW, false> edge(s_ring, wv, lane, a[NS - 2], a[NS - 1]);
    uint32_t* bp = (BP_LDS ? s_bp : g_bp) + wv * 64 + lane;
    // one step: a[] (t-1) -> a[] (t) with emissions em[]; the lane's NS backpointers leave as one dword (with the table in the
    // workspace that dword is a store like the loss's lattice row)
    ctc_for_each_step<NS, EM_LDS, false>(lp, s_lp + C, cls4, Tb, (int)C, [&](const float (&em)[NS]) {
      float n1, n2, n[NS];
      edge.neighbours(a, n1, n2);
      uint32_t word = 0;
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        float s1, s2;
        ctc_adjacent<NS, false>(a, n1, n2, i, s1, s2);
        // even states are blanks: no skip into them
        const float m = (i & 1) ? v_max3(a[i], s1, skip_ok[i] ? s2 : kDead) : v_max2(a[i], s1);
        const uint32_t back = (a[i] == m) ? 0u : ((s1 == m) ? 1u : 2u);   // stay, then step, then skip
        word |= back << (2 * i);
        n[i] = m + em[i];
      }
      edge.publish(n[NS - 2], n[NS - 1]);
      bp += RW;
      *bp = word;
#pragma unroll
      for (int i = 0; i < NS; ++i) a[i] = n[i];
      edge.barrier();
    });
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = s0 + i;
      if (s == SS - 1) s_fin[1] = a[i];
      if (s == SS - 2) s_fin[0] = a[i];
    }
  }
  __syncthreads();   // the final scores and every wave's backpointer rows (LDS or workspace) are visible to wave 0

  // ------------------------------------------------------------------ final state, backtrace
  const float v_blank = s_fin[1], v_label = s_fin[0];
  const bool end_blank = (S == 0) || (v_blank >= v_label);
  const float sc = end_blank ? v_blank : v_label;
  const bool feasible = sc > 0.5f * kDead;             // false for a dead state, -inf and NaN
  if (threadIdx.x == 0) score[b] = feasible ? sc : kNegInf;
  if (feasible && wv == 0) {
    int s = __builtin_amdgcn_readfirstlane(end_blank ? SS - 1 : SS - 2);
    const uint32_t* tab = BP_LDS ? s_bp : g_bp;
    uint32_t cur[kAlignBtRows][NWR], nxt[kAlignBtRows][NWR];
    auto fetch = [&](uint32_t (&w)[kAlignBtRows][NWR], int t_hi) {
#pragma unroll
      for (int u = 0; u < kAlignBtRows; ++u) {
        const int t = min(max(t_hi - u, 1), Tb - 1);    // rows 1 .. Tb-1 exist; a clamped row is fetched and not used
#pragma unroll
        for (int k = 0; k < NWR; ++k) w[u][k] = tab[(int64_t)t * RW + min(k, NW - 1) * 64 + lane];
      }
    };
    int mine = 0;                                       // lane l keeps the state of frame t with t % 64 == l until the flush
    if (Tb >= 2) {
      fetch(cur, Tb - 1);
      for (int t_hi = Tb - 1; t_hi >= 1; t_hi -= kAlignBtRows) {
        fetch(nxt, t_hi - kAlignBtRows);                // one chunk ahead of the walk (clamped past the start)
#pragma unroll
        for (int u = 0; u < kAlignBtRows; ++u) {
          const int t = t_hi - u;
          if (t >= 1) {  // wave-uniform
            mine = (lane == (t & 63)) ? s : mine;
            if ((t & 63) == 0 && t + lane < Tb) s_st[t + lane] = mine;
            const int widx = s >> LOG_NS;
            uint32_t x = cur[u][0];
            if (MW) {
#pragma unroll
              for (int k = 1; k < NWR; ++k) x = ((widx >> 6) == k) ? cur[u][k] : x;
            }
            const uint32_t word = __builtin_amdgcn_readlane(x, __builtin_amdgcn_readfirstlane(widx & 63));
            const int back = (int)((word >> (2 * (s & (NS - 1)))) & 3u);
            s = max(s - back, 0);
          }
        }
#pragma unroll
        for (int u = 0; u < kAlignBtRows; ++u)
#pragma unroll
          for (int k = 0; k < NWR; ++k) cur[u][k] = nxt[u][k];
      }
    }
    mine = (lane == 0) ? s : mine;                      // frame 0
    if (lane < Tb) s_st[lane] = mine;
  }
  __syncthreads();

  // ------------------------------------------------------------------ frames and spans, in parallel over frames
  for (int t = threadIdx.x; t < (int)T; t += NT) {
    int st = -1;
    float e = 0.f;
    if (feasible && t < Tb) {
      st = s_st[t];
      e = lp[(int64_t)t * C + ((st & 1) ? s_tg[st >> 1] : blank)];
      if (st & 1) {
        // an odd state that differs from the previous frame's opens label st >> 1; one that differs from the next closes it
        const int prev = t > 0 ? s_st[t - 1] : -1;
        const int next = t + 1 < Tb ? s_st[t + 1] : -1;
        if (prev != st) label_start[(int64_t)b * S_max + (st >> 1)] = t;
        if (next != st) label_end[(int64_t)b * S_max + (st >> 1)] = t + 1;
      }
    }
    frame_state[(int64_t)b * T + t] = st;
    frame_logp[(int64_t)b * T + t] = e;
  }
}

}  // namespace lasr

using namespace lasr;

extern "C" size_t lasr_ctc_align_workspace_bytes(int64_t B, int64_t T, int64_t S_max) {
  if (B <= 0 || T <= 0 || S_max < 0) return 0;
  const CtcGeom geo = ctc_geom(S_max);
  return geo.pitch ? align_up((size_t)B * align_bp_bytes(T, geo.nw), 256) : 0;
}

extern "C" int lasr_ctc_align(const float* logp, const int64_t* targets, const int32_t* in_lens, const int32_t* tgt_lens, int64_t B,
                              int64_t T, int64_t C, int64_t S_max, int blank, float* score, int32_t* frame_state, float* frame_logp,
                              int32_t* label_start, int32_t* label_end, void* workspace, size_t workspace_bytes, void* stream) {
  LASR_CHECK_ARG(logp && tgt_lens && score && frame_state && frame_logp && workspace, "lasr_ctc_align: null pointer");
  LASR_CHECK_ARG(S_max <= 0 || (targets && label_start && label_end), "lasr_ctc_align: null pointer");
  LASR_CHECK_SHAPE(B > 0 && T > 0 && C > 1 && S_max >= 0 && blank >= 0 && blank < C && T * C < (int64_t)1 << 31, "lasr_ctc_align: shape");
  const CtcGeom geo = ctc_geom(S_max);
  LASR_CHECK_SHAPE(geo.pitch != 0, "lasr_ctc_align: S_max=%lld exceeds the %d-label bound of the CTC lattice", (long long)S_max,
                   LASR_CTC_MAX_LABELS);
  if (workspace_bytes < lasr_ctc_align_workspace_bytes(B, T, S_max)) return fail(LASR_E_WORKSPACE, "lasr_ctc_align: workspace");
  // LDS budget: the label table and the ring (static), the frame states, then the emission block when it fits (ctc_em_in_lds), then
  // the backpointer table when it fits beside both
  const size_t fixed = kCtcMwMaxS * sizeof(int32_t) + kCtcLdsHeadroom + align_state_bytes(T);
  const bool em_lds = ctc_em_in_lds(T, C, fixed, logp);
  const size_t em_bytes = em_lds ? ctc_em_bytes(T, C) : 0, bp_bytes = align_bp_bytes(T, geo.nw);
  const bool bp_lds = !ctc_no_lds() && fixed + em_bytes + bp_bytes <= kLdsBytes;
  const size_t lds = em_bytes + align_state_bytes(T) + (bp_lds ? bp_bytes : 0);
  auto launch = [&](auto kernel, unsigned threads) {
    launch_lds(kernel, dim3((unsigned)B), dim3(threads), lds, as_stream(stream), logp, targets, in_lens, tgt_lens, T, C, S_max, blank, score,
               frame_state, frame_logp, label_start, label_end, static_cast<uint32_t*>(workspace));
  };
  if (geo.ns) {
    LASR_TRY(with_int<4, 8, 16>(geo.ns, [&](auto ns) {
      with_bool(em_lds, [&](auto em) {
        with_bool(bp_lds, [&](auto bp) {
          launch(ctc_align_kernel<decltype(ns)::value, false, decltype(em)::value, decltype(bp)::value>, kAlignThreads);
        });
      });
    }));
  } else {
    with_bool(em_lds, [&](auto em) {
      with_bool(bp_lds, [&](auto bp) {
        launch(ctc_align_kernel<kCtcMwNS, true, decltype(em)::value, decltype(bp)::value>, 64u * (unsigned)geo.nw);
      });
    });
  }
  LASR_LAUNCH_CHECK("ctc_align_kernel");
  return 0;
}
