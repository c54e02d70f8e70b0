// CTC lattice device code: the one lattice walk (staging, state table, emission stream, edge exchange) behind the sum-product
// recursions of the loss and the max-product recursion of forced alignment.  Users: ctc.hip (stand-alone loss kernels),
// ctc_lean.hip (large-vocabulary head, compact emissions), mel.hip (the lattice workgroups inside the feature-prefetch grid) and
// ctc_align.hip (forced alignment).  Replaces nn.CTCLoss forward (train.py:77-78,196).
#pragma once
#include "common.h"
#include <math.h>

namespace lasr {

static constexpr float kNegInf = -INFINITY;

// ------------------------------------------------------------------ CTC ------------------------
// log-sum-exp on the hardware exp2/log2 units (__expf/__logf -> v_exp_f32/v_log_f32): the recursion
// is a ~500-step dependent chain per utterance, so transcendental LATENCY is the kernel's run time
// (libm expf/logf: ~0.5 ms per step of the bench; these: ~10x less).  Arguments are in [-90, 0] and
// [1, 3]; the relative error per step (~1e-6) stays far inside the 1e-4 loss tolerance.
// Branch-free: with every input -inf the shifted sum is exp(-inf)*3 = 0 and log(0) = -inf, so no
// per-lane early exit is needed (divergent exits cost an exec-mask branch per state per step).
// Neighbour exchange of the lattice recursion on the DPP path (gfx9 wave-wide shifts, one VALU op) instead of
// ds_bpermute (an LDS round trip on the critical path of every one of the T' dependent steps):
// wave_shr1: lane i receives lane i-1, lane 0 keeps `fill`; wave_shl1: lane i receives lane i+1, lane 63 `fill`.
__device__ __forceinline__ float wave_shr1(float v, float fill) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float v, float fill) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  const float mm = (m == kNegInf) ? 0.f : m;
  return mm + __logf(__expf(a - mm) + __expf(b - mm) + __expf(c - mm));
}
__device__ __forceinline__ float lse2(float a, float b) { return lse3(a, b, kNegInf); }

// lse3 for the alpha/beta recursions on the raw transcendental units: v_exp_f32 / v_log_f32 ARE 2^x / log2(x), so
// the differences are scaled by log2(e) and the logarithm by ln(2): the same values in natural-log units (the
// rounding that matters, of m + log(sum) at |alpha| ~ 1e3, is unchanged; a pure base-2 lattice was 1.4x faster
// still but its unit conversions at that magnitude cost 30 % more gradient error against an f64 reference).
//
// The recursion is ISSUE-bound (one wave per SIMD, ~60 VALU instructions per time step), so the per-step
// instruction count is the kernel's run time.  What keeps it short:
//   * unreachable states hold the finite sentinel kDead = -1e30 instead of -inf: it absorbs every update
//     (-1e30 + log(3) + emission rounds back to -1e30), exp2 of differences against it is exactly 0, and no
//     "all three are -inf" special case (compare + two selects per state) is left in the chain;
//   * the largest term of the sum is exp(0) = 1: only the smaller ones go through the quarter-rate v_exp_f32;
//   * max3 / med3 / min3 as single instructions without the IEEE-mode canonicalisation of their inputs;
//   * alpha and beta are separate instantiations selected by a scalar branch (a per-lane `is_beta` compiled to
//     exec-mask divergence: both bodies' register shuffles ran every step);
//   * no `s < SS` masking: alpha's states >= SS never feed a lower state, beta's start dead and stay dead.
static constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
static constexpr float kDead = -1e30f;
__device__ __forceinline__ float v_max3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float v_min3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float v_med3(float a, float b, float c) { float r; asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float v_max2(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float v_min2(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

__device__ __forceinline__ float lse3_fast(float a, float b, float c) {
  const float m = v_max3(a, b, c);
  const float md = v_med3(a, b, c);
  const float lo = v_min3(a, b, c);
  const float s = 1.f + __builtin_amdgcn_exp2f((md - m) * kLog2e) + __builtin_amdgcn_exp2f((lo - m) * kLog2e);
  return fmaf(kLn2, __builtin_amdgcn_logf(s), m);
}

__device__ __forceinline__ float lse2_fast(float a, float b) {
  const float m = v_max2(a, b);
  const float lo = v_min2(a, b);
  const float s = 1.f + __builtin_amdgcn_exp2f((lo - m) * kLog2e);
  return fmaf(kLn2, __builtin_amdgcn_logf(s), m);
}

// ------------------------------------------------------------------ the lattice walk, one copy ------------------------
// One utterance's 2S+1 states sit NS = 4 / 8 / 16 per lane on one wave (S_max <= 511) or, above that, 16 per lane on NW =
// ceil((2 S_max + 1) / 1024) = 2, 3 or 4 waves: wave w owns states [1024 w, 1024 (w + 1)).  The pieces below are what the
// sum-product recursions of the loss (ctc_lattice, both directions, one- and multi-wave) and the max-product recursion of
// ctc_align.hip are built from; only the per-state operator and what a step stores are the callers' own.
static constexpr int kCtcMaxS = 512;                    // label table entries of the one-wave kernels
static constexpr int kCtcMwNS = 16;                     // multi-wave: states per lane
static constexpr int kCtcMwWaveStates = 64 * kCtcMwNS;  // 1024 states per wave
static constexpr int kCtcMwMaxWaves = 4;
static constexpr int kCtcMwMaxS = 2048;                 // label table entries (S_max <= 2047 = LASR_CTC_MAX_LABELS)
static constexpr int kCtcRingRow = 2 * (kCtcMwMaxWaves + 2);   // one slot of the edge ring: two states per wave, a sentinel entry at either end
static constexpr int kCtcRingFloats = 2 * kCtcRingRow;         // the ring: two slots

// ---- staging, by all NT threads of the workgroup that take part, before its __syncthreads
// The utterance's labels into LDS, clamped into [0, hi] (the last column of an emission row): invalid user data must not
// become an out-of-bounds device access.
__device__ __forceinline__ void ctc_load_labels(const int64_t* __restrict__ tg, int S, int64_t hi, int NT, int32_t* s_tg) {
  for (int i = threadIdx.x; i < S; i += NT) s_tg[i] = (int32_t)min(max(tg[i], (int64_t)0), hi);
}

// The utterance's emission rows 0..Tb-1 (Tb x C f32; 56 KB at T'=501, C=28) into LDS behind one pad row, with a second pad row
// after them (s_lp: (T + 2) * C floats, row t at s_lp + (t + 1) * C): coalesced 16-byte loads, 4 in flight per thread.  The
// recursion then gathers its per-state emissions from there one step ahead without an end-of-sequence clamp, so its T'
// dependent steps contain no global load and never wait on vmcnt (which also counts the lattice stores).  The pad rows are
// read one step past either end and never used.  The host checked C % 4 == 0 and the 16-byte alignment of lp (ctc_em_in_lds).
__device__ __forceinline__ void ctc_fill_emissions(const float* __restrict__ lp, int Tb, int64_t C, int NT, float* s_lp) {
  const int n4 = (int)(((int64_t)Tb * C) >> 2);
  const float4* src = reinterpret_cast<const float4*>(lp);
  float4* dst = reinterpret_cast<float4*>(s_lp + C);
  for (int i0 = threadIdx.x; i0 < n4; i0 += 4 * NT) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src[min(i0 + u * NT, n4 - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u * NT < n4) dst[i0 + u * NT] = v[u];
  }
  for (int i = threadIdx.x; i < (int)C; i += NT) {
    s_lp[i] = 0.f;
    s_lp[(int64_t)(Tb + 1) * C + i] = 0.f;
  }
}

// Chain of equal labels (for the deterministic per-class sum in the gradient kernel), after the labels are in LDS: this thread
// takes labels first, first + stride, ... (first < 0: none).  One pass over the labels finds both answers: the smallest j > i
// with the same label, and whether any j < i has it.  nx_b: the utterance's next_same [2][S_max].
__device__ __forceinline__ void ctc_label_chain(const int32_t* s_tg, int S, int first, int stride, int32_t* __restrict__ nx_b, int64_t S_max) {
  for (int i = first; i >= 0 && i < S; i += stride) {
    const int me = s_tg[i];
    int nx = -1, first_me = 1;
#pragma unroll 8
    for (int j = S - 1; j >= 0; --j) {
      const bool same = s_tg[j] == me;
      nx = (same && j > i) ? j : nx;
      first_me = (same && j < i) ? 0 : first_me;
    }
    nx_b[i] = nx;
    nx_b[S_max + i] = first_me;
  }
}

// ---- the state table of a lane whose first state is s0: cls4[] the byte offset of each state's class inside an emission row,
// skip_ok[] whether the skip transition into (alpha) / out of (beta) the state exists - between different labels only - and
// a[] the start values from the first row `row0` (t = 0, or Tb - 1 for beta): the two start states, everything else kDead.
// COMPACT: the emission matrix is the gathered one of ctc_lean.hip - row t holds the emission of label POSITION i in column i
// and the blank's in column `blank` (= S_max): the class of an odd state is its position, the skip rule still compares the
// labels themselves.
// A macro over the caller's own int cls4[NS], bool skip_ok[NS], float a[NS], not a function that takes them by reference: such
// a helper is simplified on its own before it is inlined, and the register-ring recursions (NS = 8, 16) then came out one
// s_waitcnt per step longer than with the table written in place (profiles/lattice_refactor_check.txt, section 1).  Left
// defined at the end of this header on purpose: ctc_align.hip expands it as well.
#define LASR_CTC_LATTICE_STATES(NS, BETA, COMPACT, s_tg, s0, SS, blank, row0, cls4, skip_ok, a)                 \
  _Pragma("unroll") for (int i_ = 0; i_ < (NS); ++i_) {                                                        \
    const int s_ = (s0) + i_;                                                                                  \
    int c_ = (blank);                                                                                          \
    bool sk_ = false;                                                                                          \
    if (s_ < (SS) && (s_ & 1)) {                                                                               \
      const int lab_ = (s_tg)[s_ >> 1];                                                                        \
      c_ = (COMPACT) ? (s_ >> 1) : lab_;                                                                       \
      if (!(BETA)) sk_ = s_ >= 3 ? ((s_tg)[(s_ >> 1) - 1] != lab_) : false;        /* from s-2 into s */        \
      else sk_ = (s_ + 2 < (SS)) ? ((s_tg)[(s_ >> 1) + 1] != lab_) : false;        /* from s into s+2 */        \
    }                                                                                                          \
    (cls4)[i_] = c_ * 4;                                                                                       \
    (skip_ok)[i_] = sk_;                                                                                       \
  }                                                                                                            \
  _Pragma("unroll") for (int i_ = 0; i_ < (NS); ++i_) {                                                        \
    const int s_ = (s0) + i_;                                                                                  \
    const bool start_ = (BETA) ? (s_ == (SS) - 1 || s_ == (SS) - 2) : (s_ == 0 || s_ == 1);                    \
    (a)[i_] = (start_ && s_ < (SS)) ? (row0)[(cls4)[i_] >> 2] : kDead;                                         \
  }

// ---- the emission stream: advance(em) once per step 1 .. Tb-1 (alpha: t = step, beta: t = Tb - 1 - step) with em[] the
// emissions of the lane's states at t.  lp: the utterance's emission matrix; s_rows (EM_LDS): the same in LDS, row t at
// s_rows + t * C with a pad row on either side (ctc_fill_emissions).  Every wave of a workgroup passes the same Tb.
template <int NS, bool EM_LDS, bool BETA, int kPre = 8, class Step>
__device__ __forceinline__ void ctc_for_each_step(const float* __restrict__ lp, const float* s_rows, const int (&cls4)[NS], int Tb, int C,
                                                  Step&& advance) {
  const int t_first = BETA ? Tb - 1 : 0;
  constexpr int dt = BETA ? -1 : 1;
  float em[NS];
  if (EM_LDS) {
    const char* row = reinterpret_cast<const char*>(s_rows) + (int64_t)(t_first + dt) * C * 4;
    const int drow = dt * C * 4;
    float nx[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) nx[i] = *reinterpret_cast<const float*>(row + cls4[i]);
    for (int step = 1; step < Tb; ++step) {
#pragma unroll
      for (int i = 0; i < NS; ++i) em[i] = nx[i];
      row += drow;                                   // next step's emissions: issued before this step's arithmetic
#pragma unroll                                       // (the last one reads the pad row)
      for (int i = 0; i < NS; ++i) nx[i] = *reinterpret_cast<const float*>(row + cls4[i]);
      advance(em);
    }
  } else {
    // Emissions are fetched kPre steps ahead into a register ring.  On CDNA4 s_waitcnt vmcnt counts
    // stores as well as loads, in issue order: with a one-step prefetch every step would also wait for
    // the previous step's stores (lattice rows, backpointer dwords) to retire (~0.7 us).  Eight steps of slack hide both (kPre:
    // the ring is kPre * NS registers; ctc_align_long.hip's eight-wave form has room for four steps).
    float ring[kPre][NS];
#pragma unroll
    for (int u = 0; u < kPre; ++u)
#pragma unroll
      for (int i = 0; i < NS; ++i)
        ring[u][i] = (1 + u < Tb) ? lp[(int64_t)(t_first + dt * (1 + u)) * C + (cls4[i] >> 2)] : 0.f;
    for (int step0 = 1; step0 < Tb; step0 += kPre) {
#pragma unroll
      for (int u = 0; u < kPre; ++u) {
        const int step = step0 + u;
        if (step < Tb) {  // wave-uniform, so a real branch; MW: the same in every wave of the workgroup, as the step's barrier needs
          const int t = t_first + dt * step;
#pragma unroll
          for (int i = 0; i < NS; ++i) em[i] = ring[u][i];
          {   // unconditional refill from a clamped row: a load inside a branch is drained (s_waitcnt vmcnt(0)) at the branch's
              // join, which put the memory round trip back on every step's critical path
            const int tq = BETA ? max(t - kPre, 0) : min(t + kPre, Tb - 1);
#pragma unroll
            for (int i = 0; i < NS; ++i) ring[u][i] = lp[(int64_t)tq * C + (cls4[i] >> 2)];
          }
          advance(em);
        }
      }
    }
  }
}

// ---- the edge exchange: where the two states below a lane's first (alpha) / above its last (beta) come from.  Inside a wave
// they are the neighbouring lane's, one DPP shift each.  Lane 0 (alpha) / 63 (beta) has no such lane:
//   !MW  it gets the fill kDead - nothing feeds the lattice's first states from below or its last from above.  No LDS traffic,
//        no barrier.
//   MW   it gets the previous step's two edge states of the neighbouring wave (alpha: wave w-1's top two, beta: wave w+1's
//        bottom two).  They pass through a two-slot LDS ring indexed by the parity of the step: step k reads the slot written
//        at step k-1 and writes the other, then one s_barrier.  The barrier of step k orders step k's writes before step k+1's
//        reads and step k's reads before step k+1's overwrite of the same slot two steps later, so one barrier per step
//        suffices without skewing the waves against each other.  The barrier waits on LDS only (lds_barrier, common.h): the
//        stores and the emission prefetches of the step stay in flight across it.  Ring entry 0 (alpha) / NW + 1 (beta) is a
//        permanent kDead sentinel: the outermost waves take it as the fill the one-wave form gives lane 0 / lane 63, so with
//        all live states inside wave 0 the results are bit-identical to it.
// s_ring: kCtcRingFloats floats, every entry kDead on entry (ctc_edge_init).  Every wave of the workgroup runs the same number
// of steps: one barrier at construction and one per barrier().
template <bool MW, bool BETA>
struct CtcEdge {
  float* s_ring;
  int r_in, r_out, par;   // the neighbour's ring entry, this wave's, and the slot of the previous step
  bool owner;             // the lane that holds the wave's edge states
  // lo, hi: the lane's edge states of step 0 (alpha: its top two, beta: its bottom two, in state order)
  __device__ __forceinline__ CtcEdge(float* ring, int wv, int lane, float lo, float hi)
      : s_ring(ring), r_in(BETA ? 2 * (wv + 2) : 2 * wv), r_out(2 * (wv + 1)), par(0), owner(lane == (BETA ? 0 : 63)) {
    if (MW) {
      if (owner) { s_ring[r_out] = lo; s_ring[r_out + 1] = hi; }
      lds_barrier();
    }
  }
  // n1 / n2: for each lane the state one / two below its a[0] (alpha), above its a[NS-1] (beta)
  template <int NS>
  __device__ __forceinline__ void neighbours(const float (&a)[NS], float& n1, float& n2) const {
    float f_lo = kDead, f_hi = kDead;
    if (MW) {
      const float* rin = s_ring + par * kCtcRingRow + r_in;
      f_lo = rin[0];
      f_hi = rin[1];
    }
    if (!BETA) {
      n1 = wave_shr1(a[NS - 1], f_hi);
      n2 = wave_shr1(a[NS - 2], f_lo);
    } else {
      n1 = wave_shl1(a[0], f_lo);
      n2 = wave_shl1(a[1], f_hi);
    }
  }
  // the new edge states of this step, for the neighbour's next one
  __device__ __forceinline__ void publish(float lo, float hi) {
    if (MW) {
      par ^= 1;
      float* rout = s_ring + par * kCtcRingRow + r_out;
      if (owner) { rout[0] = lo; rout[1] = hi; }
    }
  }
  __device__ __forceinline__ void barrier() const {
    if (MW) lds_barrier();
  }
};
// The ring's entries to kDead and the two cells s_fin, through which the last frame's states 2S-1 and 2S reach wave 0, to -inf
// (what a cell that no lane writes must read as; what the lanes leave there is each caller's own), before the workgroup's __syncthreads.
__device__ __forceinline__ void ctc_edge_init(float* s_ring, float* s_fin) {
  if (threadIdx.x < kCtcRingFloats) s_ring[threadIdx.x] = kDead;
  if (threadIdx.x < 2) s_fin[threadIdx.x] = kNegInf;
}
// The predecessors (alpha: s-1, s-2) / successors (beta: s+1, s+2) of a lane's state i: its own registers, or n1 / n2 of
// CtcEdge::neighbours across the lane's edge.
template <int NS, bool BETA>
__device__ __forceinline__ void ctc_adjacent(const float (&a)[NS], float n1, float n2, int i, float& s1, float& s2) {
  if (!BETA) {
    // i==0: s-1 is the previous lane's last state, s-2 its second to last; i==1: s-2 is the previous lane's last
    s1 = i >= 1 ? a[i - 1] : n1;
    s2 = (i == 0) ? n2 : (i == 1 ? n1 : a[i - 2]);
  } else {
    s1 = i + 1 < NS ? a[i + 1] : n1;
    s2 = (i + 2 < NS) ? a[i + 2] : (i + 2 == NS ? n1 : n2);
  }
}

// ---- One direction of the sum-product lattice for one utterance, by one wave (!MW: wv = 0, NW = 1, s_ring = s_fin = nullptr)
// or as wave `wv` of the NW that share it (MW: NS = 16; s_ring / s_fin as ctc_edge_init left them; the barrier count is Tb - 1,
// + 1 for the nll).  s_tg: the utterance's targets in LDS; lp / s_rows / C: ctc_for_each_step; out: the utterance's lattice,
// rows of 64 NS NW floats.  Stored rows hold kDead for unreachable states and unspecified values for s >= 2S+1 (the gradient
// kernel reads s < 2S+1 only).
template <int NS, bool MW, bool EM_LDS, bool BETA, bool COMPACT = false>
__device__ __forceinline__ void ctc_lattice(const float* __restrict__ lp, const float* s_rows, const int32_t* s_tg, int lane, int wv, int NW,
                                            int Tb, int S, int C, int blank, float* __restrict__ out, float* s_ring, float* s_fin,
                                            float* __restrict__ nll_b) {
  static_assert(!MW || NS == kCtcMwNS, "the multi-wave form holds 16 states per lane");
  const int SP = 64 * NS * NW;
  const int SS = 2 * S + 1;
  const int s0 = wv * (64 * NS) + lane * NS;           // this lane's first state
  const int t_first = BETA ? Tb - 1 : 0;
  constexpr int dt = BETA ? -1 : 1;
  int cls4[NS];
  bool skip_ok[NS];
  float a[NS];
  const float* row0 = lp + (int64_t)t_first * C;
  LASR_CTC_LATTICE_STATES(NS, BETA, COMPACT, s_tg, s0, SS, blank, row0, cls4, skip_ok, a)
  float* o = out + (int64_t)t_first * SP + s0;
#pragma unroll
  for (int i = 0; i < NS; ++i) o[i] = a[i];
  CtcEdge<MW, BETA> edge(s_ring, wv, lane, BETA ? a[0] : a[NS - 2], BETA ? a[1] : a[NS - 1]);
  // one recursion step: a[] (t - dt) -> a[] (t) with emissions em[], lattice row stored
  ctc_for_each_step<NS, EM_LDS, BETA>(lp, s_rows, cls4, Tb, C, [&](const float (&em)[NS]) {
    float n1, n2, n[NS];
    edge.neighbours(a, n1, n2);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      float s1, s2;
      ctc_adjacent<NS, BETA>(a, n1, n2, i, s1, s2);
      // even states are blanks (NS is even, so the parity of s is the parity of i): no skip transition, two terms
      n[i] = ((i & 1) ? lse3_fast(a[i], s1, skip_ok[i] ? s2 : kDead) : lse2_fast(a[i], s1)) + em[i];
    }
    edge.publish(BETA ? n[0] : n[NS - 2], BETA ? n[1] : n[NS - 1]);
    o += dt * SP;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      a[i] = n[i];
      o[i] = n[i];
    }
    edge.barrier();
  });
  if (!BETA) {
    // ll = lse(alpha_{T-1}(SS-1), alpha_{T-1}(SS-2)); two candidate states, in at most two lanes
    float v = kNegInf;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = s0 + i;
      if ((s == SS - 1 || s == SS - 2) && a[i] > 0.5f * kDead) v = lse2(v, a[i]);
    }
    if (MW) {
      // the two lanes may sit in two waves: they leave their lse2 partial in s_fin, the lane of SS-1 in [1], a different lane
      // holding SS-2 in [0], and wave 0 reduces as the one-wave form does (the max and a sum of at most two non-zero terms do
      // not depend on which lanes hold them)
      bool own1 = false, own2 = false;
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        own1 |= s0 + i == SS - 1;
        own2 |= s0 + i == SS - 2;
      }
      if (own1) s_fin[1] = v;
      else if (own2) s_fin[0] = v;
      lds_barrier();
      if (wv != 0) return;
      v = lane < 2 ? s_fin[lane] : kNegInf;
    }
    const float m = wave_max(v);
    float e = (v == kNegInf) ? 0.f : expf(v - m);
    e = wave_sum(e);
    if (lane == 0) *nll_b = (m == kNegInf) ? INFINITY : -(m + logf(e));
  }
}

// ---- the two shells: how an utterance's two directions map onto workgroups
// One-wave form.  Workspace layout per utterance: alpha [T][SP], beta [T][SP] (SP = 64*NS), then next_same [2][S_max] int32.
// grid: B blocks (wave 0: alpha, wave 1: beta).  b: utterance; NT: threads of the workgroup that take part (128 in the
// stand-alone kernel, 256 inside the fused mel + CTC grid: the upper waves help with the LDS fill and take the label chain,
// then leave); s_tg: kCtcMaxS ints, s_lp (EM_LDS): (T + 2) * C floats.  Large vocabularies (C=4334) keep the register ring.
template <int NS, bool EM_LDS, int NT, bool COMPACT = false>
__device__ __forceinline__ void ctc_alpha_beta_body(const float* __restrict__ logp, const int64_t* __restrict__ targets,
                                                    const int32_t* __restrict__ in_lens, const int32_t* __restrict__ tgt_lens,
                                                    int64_t T, int64_t C, int64_t S_max, int blank, float* __restrict__ alpha,
                                                    float* __restrict__ beta, int32_t* __restrict__ next_same,
                                                    float* __restrict__ nll, int b, int32_t* s_tg, float* s_lp) {
  constexpr int SP = 64 * NS;
  const int lane = threadIdx.x & 63;
  const int Tb = in_lens[b];
  const int S = tgt_lens[b];
  const float* lp = logp + (int64_t)b * T * C;
  ctc_load_labels(targets + (int64_t)b * S_max, S, COMPACT ? 0x7fffffff : C - 1, NT, s_tg);
  if (EM_LDS && Tb > 0) ctc_fill_emissions(lp, Tb, C, NT, s_lp);
  __syncthreads();
  // the label chain by the helper waves where the workgroup has any: as two O(S) loops of dependent-latency LDS reads per label on
  // the lattice waves they stood 6.5 us (S = 100) in front of the recursion (phase stamps, round 5)
  constexpr int kChainT0 = NT > 128 ? 128 : 0, kChainN = NT > 128 ? NT - 128 : NT;
  ctc_label_chain(s_tg, S, (int)threadIdx.x - kChainT0, kChainN, next_same + (int64_t)b * S_max * 2, S_max);
  if (Tb <= 0) {
    if (threadIdx.x == 0) nll[b] = (S == 0) ? 0.f : INFINITY;
    return;
  }
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // scalar: real branches
  if (wv >= 2) return;                                                        // helper waves of a wider workgroup
  const bool is_beta = wv != 0;
  if (is_beta)
    ctc_lattice<NS, false, EM_LDS, true, COMPACT>(lp, s_lp + C, s_tg, lane, 0, 1, Tb, S, (int)C, blank, beta + (int64_t)b * T * SP, nullptr,
                                                  nullptr, nullptr);
  else
    ctc_lattice<NS, false, EM_LDS, false, COMPACT>(lp, s_lp + C, s_tg, lane, 0, 1, Tb, S, (int)C, blank, alpha + (int64_t)b * T * SP, nullptr,
                                                   nullptr, nll + b);
}

// Multi-wave form (S_max > 511).  Workspace layout per utterance: alpha [T][1024 NW], beta [T][1024 NW], then next_same
// [2][S_max] int32 (as the one-wave form, with the wider row).  grid: 2B workgroups of 64 NW threads, workgroup 2b + 0 runs
// alpha, 2b + 1 beta, so that each barrier couples only the waves of one recursion.  The label chain is split between the two.
// s_tg: kCtcMwMaxS ints; s_lp (EM_LDS): (T + 2) * C floats; s_ring: kCtcRingFloats floats, s_fin: 2.
template <bool EM_LDS, bool COMPACT>
__device__ __forceinline__ void ctc_alpha_beta_mw_body(const float* __restrict__ logp, const int64_t* __restrict__ targets,
                                                       const int32_t* __restrict__ in_lens, const int32_t* __restrict__ tgt_lens,
                                                       int64_t T, int64_t C, int64_t S_max, int blank, float* __restrict__ alpha,
                                                       float* __restrict__ beta, int32_t* __restrict__ next_same,
                                                       float* __restrict__ nll, int32_t* s_tg, float* s_lp, float* s_ring, float* s_fin) {
  const int NT = (int)blockDim.x;
  const int NW = NT >> 6;
  const int SP = kCtcMwWaveStates * NW;
  const int b = (int)(blockIdx.x >> 1);
  const bool is_beta = (blockIdx.x & 1) != 0;
  const int lane = threadIdx.x & 63;
  const int Tb = in_lens[b];
  const int S = tgt_lens[b];
  const float* lp = logp + (int64_t)b * T * C;
  ctc_load_labels(targets + (int64_t)b * S_max, S, COMPACT ? 0x7fffffff : C - 1, NT, s_tg);
  ctc_edge_init(s_ring, s_fin);
  if (EM_LDS && Tb > 0) ctc_fill_emissions(lp, Tb, C, NT, s_lp);
  __syncthreads();
  // labels i of the alpha workgroup's half, then the beta workgroup's
  ctc_label_chain(s_tg, S, (int)threadIdx.x + (is_beta ? NT : 0), 2 * NT, next_same + (int64_t)b * S_max * 2, S_max);
  if (Tb <= 0) {
    if (!is_beta && threadIdx.x == 0) nll[b] = (S == 0) ? 0.f : INFINITY;
    return;
  }
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (is_beta)
    ctc_lattice<kCtcMwNS, true, EM_LDS, true, COMPACT>(lp, s_lp + C, s_tg, lane, wv, NW, Tb, S, (int)C, blank, beta + (int64_t)b * T * SP,
                                                       s_ring, s_fin, nullptr);
  else
    ctc_lattice<kCtcMwNS, true, EM_LDS, false, COMPACT>(lp, s_lp + C, s_tg, lane, wv, NW, Tb, S, (int)C, blank, alpha + (int64_t)b * T * SP,
                                                        s_ring, s_fin, nll + b);
}

// Lattice geometry for a label width S_max: ns = 4 / 8 / 16 states per lane on one wave (S_max <= 511), or 0 with nw = 2..4
// waves of 16 states per lane (S_max <= 2047); pitch = floats per lattice row, 0 above the bound.
struct CtcGeom {
  int ns, nw;
  int64_t pitch;
};
static inline CtcGeom ctc_geom(int64_t S_max) {
  const int64_t ss = 2 * S_max + 1;
  if (ss <= 64 * 4) return {4, 1, 64 * 4};
  if (ss <= 64 * 8) return {8, 1, 64 * 8};
  if (ss <= 64 * 16) return {16, 1, 64 * 16};
  if (S_max <= LASR_CTC_MAX_LABELS) {
    const int nw = (int)((ss + kCtcMwWaveStates - 1) / kCtcMwWaveStates);
    return {0, nw, (int64_t)kCtcMwWaveStates * nw};
  }
  return {0, 0, 0};
}

// The lattice workspace  alpha [B][T][pitch] | beta [B][T][pitch] | next_same [B][S_max][2]  over `ws`: its size and its layout, for
// lasr_ctc_workspace_bytes and for every launcher that fills or reads a lattice.
struct CtcWorkspace {
  CtcGeom geo;
  float* alpha; float* beta; int32_t* next_same;
  size_t bytes;                                     // 0 above the label bound
  CtcWorkspace(void* ws, int64_t B, int64_t T, int64_t S_max) : geo(ctc_geom(S_max)) {
    const size_t ab = (size_t)B * T * geo.pitch, lattice = align_up(2 * ab * sizeof(float), 256);
    const uintptr_t base = reinterpret_cast<uintptr_t>(ws);
    alpha = reinterpret_cast<float*>(base);
    beta = reinterpret_cast<float*>(base + ab * sizeof(float));
    next_same = reinterpret_cast<int32_t*>(base + lattice);
    bytes = geo.pitch ? lattice + align_up((size_t)B * (S_max > 0 ? S_max : 1) * 2 * sizeof(int32_t), 256) : 0;
  }
};

// Emission rows in LDS?  One utterance's (T + 2) x cols f32 block (a pad row on either side) has to fit `lds_total` beside
// `other_lds`, the bytes of LDS the kernel uses anyway (label table, ring, headroom), and its rows are read as 16-byte vectors.
// LASR_CTC_NO_LDS (A/B switch, read once per process) answers no for every lattice kernel.
static constexpr size_t kCtcLdsHeadroom = 2 * 1024;   // kept free beside the emissions and the label table in every budget below
inline bool ctc_no_lds() {
  static const bool off = getenv("LASR_CTC_NO_LDS") != nullptr;
  return off;
}
__host__ __device__ static inline size_t ctc_em_bytes(int64_t T, int64_t cols) { return (size_t)(T + 2) * cols * sizeof(float); }
static inline bool ctc_em_in_lds(int64_t T, int64_t cols, size_t other_lds, const void* em, size_t lds_total = kLdsBytes) {
  return !ctc_no_lds() && cols % 4 == 0 && reinterpret_cast<uintptr_t>(em) % 16 == 0 && ctc_em_bytes(T, cols) + other_lds <= lds_total;
}

// ctc.hip
int launch_ctc_grad(const float* logp, const int64_t* targets, const int32_t* in_lens, const int32_t* tgt_lens, int64_t B, int64_t T,
                    int64_t C, int64_t S_max, int blank, const float* nll, float* grad, const float* gscale, void* workspace,
                    void* stream);

}  // namespace lasr
