// Long-recording CTC forced alignment: the banded Viterbi member of the lattice family of ctc_lattice.h.  An hour of audio is
// T' ~ 180 000 frames and ~50 000 labels: the full (T, 2S+1) lattice of ctc_align.hip is 1.8e10 cells, so only a band of W states
// that follows the path is alive per frame.  The walk's pieces are the family's (the state table LASR_CTC_LATTICE_STATES, the
// emission stream ctc_for_each_step, the DPP neighbour shifts, max3 and the tie rule of ctc_align.hip); this file keeps the band:
// where it sits, which lanes it reassigns when it moves, the circular edge exchange, the 64-bit tables and the backtrace.
//
// Definition (include/lasr.h, lasr_ctc_align_long; tests/helpers/ctc_align_long_oracle.py is the same in numpy): the recursion,
// tie rule, end rule and outputs of lasr_ctc_align, with
//   frame t keeps states [lo_t, lo_t + W); lo_0 = 0; lo changes only at frames t0 that are positive multiples of R = 32, where
//     a      = the live state (> -5e29, < 2S+1) of row t0-1 with the largest value, the lowest such state; lo_prev when none
//     centre = floor((a - W/2) / G) * G,  G = 64
//     reach  = ceil((s_min(te) - (W-1)) / G) * G,  te = min(t0 + R - 1, Tb - 1),  s_min(t) = 2S-1 - 2 (Tb-1-t)
//     lo     = min(max(lo_prev, centre, reach), ceil(max(0, 2S+1 - W) / G) * G)
//   a candidate read from a state outside the previous frame's band is dead; states >= 2S+1 are dead.
//
// Geometry.  One workgroup per recording.  The band's W states sit NS = 16 per lane on W / 1024 waves (W a multiple of 1024, up
// to 8 waves) or NS = 4 per lane on W / 256 waves (the other multiples of 256, up to 16 waves).  State s lives in SLOT s mod W:
// slot p is lane (p / NS) % 64 of wave p / (64 NS).  When the band moves up by d (a multiple of G, so whole lanes) the d / NS
// lanes whose states left it take the d states that entered it - their values become dead, their labels, class offsets and skip
// flags are reloaded from global memory - and every other lane keeps its registers: a move rotates the band through the lanes and
// copies no value.  The price is that the slots are a ring: the lane below wave 0's lane 0 is the last wave's lane 63 (CtcEdge's
// ring has a dead sentinel there), and the lane that holds state lo takes no neighbour at all - except in the first step after a
// move, where lo-1 and lo-2 were inside the previous band: it takes the values they had before their lane was reassigned.
// Emissions come from global memory through the register ring of ctc_for_each_step, one call per period of R frames (the class
// offsets of a lane are constant inside a period): each period refills the ring once, one exposed memory round trip per 32 frames.
// One LDS barrier per step (none with one wave), two more at a period's start for the argmax across waves.
// Backpointers: 2 bits per SLOT, a row is W / 4 bytes at (b T + t) W / 4 of the workspace - the same dword image for both NS.
// Backtrace: wave 0 walks frames Tb-1 .. 1 with the state in a scalar register.  The state falls by at most 2 per frame, so the
// dwords a chunk of 8 rows can need are known 6 chunks ahead to within 8 dwords per row: lane 8u + k fetches, for row u of the
// chunk, the dword k below the one the state was in when the fetch was issued.  Six chunks are in flight; the dependent chain per
// frame is v_readlane + shift + subtract, as in ctc_align.hip.  Frame states go straight to frame_state, 64 per store.
// Every offset into logp, the outputs and the workspace is 64-bit: T * C and T * W are not bounded by 2^31 here.
#include "ctc_lattice.h"

namespace lasr {

static constexpr int kBandG = 64;            // granule of the band origin, states
static constexpr int kBandR = 32;            // period of the band moves, frames
static constexpr int kBandMaxWaves = 16;
static constexpr int kBandBtRows = 8;        // backtrace: rows per chunk, dwords fetched per row, chunks in flight
static constexpr int kBandBtCols = 8;
static constexpr int kBandBtAhead = 6;       // (2 * 8 * kBandBtAhead + 14 + 15) / 16 < kBandBtCols: the wanted dword is among the fetched

// the recording's labels in global memory, clamped into an emission row as ctc_load_labels clamps them: what
// LASR_CTC_LATTICE_STATES indexes where the other kernels pass their LDS table
struct BandLabels {
  const int64_t* tg;
  int64_t hi;
  __device__ __forceinline__ int operator[](int i) const { return (int)min(max(tg[i], (int64_t)0), hi); }
};

// The edge exchange of CtcEdge (ctc_lattice.h) on a ring of slots: the two states below a lane's first come from the lane
// below by one DPP shift each; lane 0 takes the previous step's top two states of the wave below, wave 0 those of the LAST wave
// (one wave: its own lane 63, by v_readlane).  MW: through a two-slot LDS ring indexed by the step's parity, one lds_barrier per
// step, by the argument of CtcEdge.
template <int NS, bool MW>
struct BandEdge {
  float (*ring)[kBandMaxWaves][2];
  int wv, below, par;
  bool owner;
  __device__ __forceinline__ BandEdge(float (*r)[kBandMaxWaves][2], int w, int NW, int lane, float lo, float hi)
      : ring(r), wv(w), below((w + NW - 1) % NW), par(0), owner(lane == 63) {
    if (MW) {
      if (owner) { ring[0][wv][0] = lo; ring[0][wv][1] = hi; }
      lds_barrier();
    }
  }
  __device__ __forceinline__ void neighbours(const float (&a)[NS], float& n1, float& n2) const {
    float f_lo, f_hi;
    if (MW) {
      f_lo = ring[par][below][0];
      f_hi = ring[par][below][1];
    } else {
      f_lo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a[NS - 2]), 63));
      f_hi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a[NS - 1]), 63));
    }
    n1 = wave_shr1(a[NS - 1], f_hi);
    n2 = wave_shr1(a[NS - 2], f_lo);
  }
  __device__ __forceinline__ void publish(float lo, float hi) {
    if (MW) {
      par ^= 1;
      if (owner) { ring[par][wv][0] = lo; ring[par][wv][1] = hi; }
    }
  }
  // the owner lane was reassigned: what it published for the previous frame belongs to states that left the band
  __device__ __forceinline__ void kill() const {
    if (MW && owner) { ring[par][wv][0] = kDead; ring[par][wv][1] = kDead; }
  }
  __device__ __forceinline__ void barrier() const {
    if (MW) lds_barrier();
  }
};

// WIDE: more than four waves of NS = 16 (W > 4096): 256 registers per lane instead of 512, so the emission ring is four steps deep
template <int NS, bool MW, bool WIDE>
__global__ __launch_bounds__(NS == 4 ? 1024 : (WIDE ? 512 : 256)) void ctc_align_long_kernel(
    const float* __restrict__ logp, const int64_t* __restrict__ targets, const int32_t* __restrict__ in_lens,
    const int32_t* __restrict__ tgt_lens, int64_t T, int64_t C, int64_t S_max, int blank, int W, float* __restrict__ score,
    int32_t* __restrict__ frame_state, float* __restrict__ frame_logp, int32_t* __restrict__ label_start,
    int32_t* __restrict__ label_end, int32_t* __restrict__ status, int32_t* __restrict__ band_lo, uint32_t* __restrict__ bp_ws) {
  __shared__ float s_ring[2][kBandMaxWaves][2];
  __shared__ float s_redv[kBandMaxWaves];
  __shared__ int s_reds[kBandMaxWaves];
  __shared__ float s_fin[2];
  __shared__ int s_rep;
  const int NT = (int)blockDim.x;
  const int NW = NT >> 6;
  const int b = (int)blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int Tb = in_lens ? min(max(in_lens[b], 0), (int)T) : (int)T;
  const int S = min(max(tgt_lens[b], 0), (int)S_max);
  const int SS = 2 * S + 1;
  const float* lp = logp + (int64_t)b * T * C;
  const BandLabels labs{targets + (int64_t)b * S_max, C - 1};
  const int RWD = W >> 4;                               // dwords per backpointer row
  uint32_t* g_bp = bp_ws + (int64_t)b * T * RWD;
  int32_t* fs = frame_state + (int64_t)b * T;
  float* flp = frame_logp + (int64_t)b * T;
  int32_t* bl = band_lo + (int64_t)b * T;
  int32_t* l_start = label_start + (int64_t)b * S_max;
  int32_t* l_end = label_end + (int64_t)b * S_max;

  for (int i = threadIdx.x; i < (int)S_max; i += NT) {   // spans of labels the path does not open stay -1
    l_start[i] = -1;
    l_end[i] = -1;
  }
  if (threadIdx.x < 2 * kBandMaxWaves * 2) (&s_ring[0][0][0])[threadIdx.x] = kDead;
  if (threadIdx.x < 2) s_fin[threadIdx.x] = kNegInf;    // v[Tb-1][2S-1], v[Tb-1][2S]: -inf where the last band does not hold them
  if (threadIdx.x == 0) s_rep = 0;
  __syncthreads();
  if (Tb <= 0) {                                        // workgroup-uniform: no frame, so no path unless there is no label either
    if (threadIdx.x == 0) {
      score[b] = (S == 0) ? 0.f : kNegInf;
      status[b] = (S == 0) ? 0 : 1;
    }
    for (int t = threadIdx.x; t < (int)T; t += NT) {
      fs[t] = -1;
      flp[t] = 0.f;
      bl[t] = -1;
    }
    return;
  }

  // ------------------------------------------------------------------ recursion
  {
    const int p0 = (wv * 64 + lane) * NS;               // this lane's first slot
    int lo = 0, s0 = p0;                                // the band's origin; this lane's first state: s0 = p0 (mod W), lo <= s0 < lo + W
    int cls4[NS];
    bool skip_ok[NS];
    float a[NS];
    LASR_CTC_LATTICE_STATES(NS, false, false, labs, s0, SS, blank, lp, cls4, skip_ok, a)
    BandEdge<NS, MW> edge(s_ring, wv, NW, lane, a[NS - 2], a[NS - 1]);
    float ff1 = kDead, ff2 = kDead;                     // what the lane of state lo takes for lo-1 / lo-2 in the next step
    if (threadIdx.x == 0) bl[0] = 0;
    int t0 = 1;
    while (t0 < Tb) {                                   // one period: frames [t0, t1), band origin constant
      const int t1 = min((t0 / kBandR + 1) * kBandR, Tb);
      if (t0 % kBandR == 0) {
        // the argmax of row t0-1: per lane in state order (strictly greater: the lowest state wins), then across lanes and
        // waves with the state as the tie-break - lanes are not in state order on the ring of slots
        float bv = kDead;
        int bs = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const bool better = a[i] > 0.5f * kDead && s0 + i < SS && a[i] > bv;
          bv = better ? a[i] : bv;
          bs = better ? s0 + i : bs;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int os = __shfl_xor(bs, o, 64);
          const bool take = ov > bv || (ov == bv && os < bs);
          bv = take ? ov : bv;
          bs = take ? os : bs;
        }
        float o1, o2;                                   // row t0-1's two states below each lane, before any lane is reassigned
        edge.neighbours(a, o1, o2);
        if (MW) {
          if (lane == 0) { s_redv[wv] = bv; s_reds[wv] = bs; }
          lds_barrier();
          bv = s_redv[0];
          bs = s_reds[0];
          for (int k = 1; k < NW; ++k) {
            const float ov = s_redv[k];
            const int os = s_reds[k];
            const bool take = ov > bv || (ov == bv && os < bs);
            bv = take ? ov : bv;
            bs = take ? os : bs;
          }
        }
        const int am = __builtin_amdgcn_readfirstlane(bs == 0x7fffffff ? lo : bs);
        const int te = min(t0 + kBandR - 1, Tb - 1);
        const int64_t s_min = 2 * (int64_t)S - 1 - 2 * (int64_t)(Tb - 1 - te);
        // negative centre / reach lose against lo >= 0 anyway: clamped at 0, so that the divisions round as floor and ceil
        const int centre = max(am - W / 2, 0) / kBandG * kBandG;
        const int reach = (int)((max(s_min - (W - 1), (int64_t)0) + kBandG - 1) / kBandG * kBandG);
        const int top = (max(SS - W, 0) + kBandG - 1) / kBandG * kBandG;
        const int lo_new = min(max(max(lo, centre), reach), top);
        if (lo_new != lo) {                             // workgroup-uniform
          const int s0n = p0 + W * ((lo_new - p0 + W - 1) / W);
          if (s0n == lo_new) {                          // lo_new-1 and lo_new-2 were in the previous band unless it jumped past them
            const bool in_prev = lo_new - lo <= W;
            ff1 = in_prev ? o1 : kDead;
            ff2 = in_prev ? o2 : kDead;
          }
          if (s0n != s0) {                              // this lane's states left the band: it takes the ones that entered, dead
            s0 = s0n;
            LASR_CTC_LATTICE_STATES(NS, false, false, labs, s0, SS, blank, lp, cls4, skip_ok, a)
            edge.kill();
          }
          lo = lo_new;
        }
        edge.barrier();                                 // the dead edges before the next step reads them; s_red before its reuse
      }
      for (int t = t0 + (int)threadIdx.x; t < t1; t += NT) bl[t] = lo;
      const bool first = s0 == lo;
      char* bp = reinterpret_cast<char*>(g_bp + (int64_t)(t0 - 1) * RWD) + (wv * 64 + lane) * (NS / 4);
      const int64_t bp_pitch = (int64_t)RWD * 4;
      // one step: a[] (t-1) -> a[] (t) with emissions em[]; the lane's NS backpointers leave as one dword (NS = 16) or byte (4)
      ctc_for_each_step<NS, false, false, WIDE ? 4 : 8>(lp + (int64_t)(t0 - 1) * C, nullptr, cls4, t1 - t0 + 1, (int)C, [&](const float (&em)[NS]) {
        float n1, n2, n[NS];
        edge.neighbours(a, n1, n2);
        n1 = first ? ff1 : n1;
        n2 = first ? ff2 : n2;
        ff1 = kDead;
        ff2 = kDead;
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          float s1, s2;
          ctc_adjacent<NS, false>(a, n1, n2, i, s1, s2);
          const float m = (i & 1) ? v_max3(a[i], s1, skip_ok[i] ? s2 : kDead) : v_max2(a[i], s1);
          const uint32_t back = (a[i] == m) ? 0u : ((s1 == m) ? 1u : 2u);   // stay, then step, then skip
          word |= back << (2 * i);
          n[i] = m + em[i];
        }
        edge.publish(n[NS - 2], n[NS - 1]);
        bp += bp_pitch;
        if (NS == 16) *reinterpret_cast<uint32_t*>(bp) = word;
        else *reinterpret_cast<uint8_t*>(bp) = (uint8_t)word;
#pragma unroll
        for (int i = 0; i < NS; ++i) a[i] = n[i];
        edge.barrier();
      });
      t0 = t1;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = s0 + i;
      if (s == SS - 1) s_fin[1] = a[i];
      if (s == SS - 2) s_fin[0] = a[i];
    }
  }
  __syncthreads();   // the final scores and every wave's backpointer rows are visible to wave 0

  // ------------------------------------------------------------------ final state, status, backtrace
  const float v_blank = s_fin[1], v_label = s_fin[0];
  const bool end_blank = (S == 0) || (v_blank >= v_label);
  const float sc = end_blank ? v_blank : v_label;
  const bool feasible = sc > 0.5f * kDead;             // false for a dead state, -inf and NaN
  if (!feasible) {                                     // workgroup-uniform: infeasible by count, or lost by the band?
    int rep = 0;
    for (int i = 1 + (int)threadIdx.x; i < S; i += NT) rep += labs[i] == labs[i - 1];
    if (rep) atomicAdd(&s_rep, rep);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    score[b] = feasible ? sc : kNegInf;
    status[b] = feasible ? 0 : ((int64_t)Tb < (int64_t)S + s_rep ? 1 : 2);
  }
  if (feasible && wv == 0) {
    int s = __builtin_amdgcn_readfirstlane(end_blank ? SS - 1 : SS - 2);
    const int u = lane >> 3, k = lane & 7;
    uint32_t x[kBandBtAhead];
    int d[kBandBtAhead];                                // the dword the state was in when chunk c's fetch was issued
    auto fetch = [&](int t_hi, int s_now, int& d0) -> uint32_t {
      d0 = s_now >> 4;
      const int t = min(max(t_hi - u, 1), Tb - 1);      // rows 1 .. Tb-1 exist; a clamped row is fetched and not used
      return g_bp[(int64_t)t * RWD + (max(d0 - k, 0) % RWD)];
    };
    int mine = 0;                                       // lane l keeps the state of frame t with t % 64 == l until the flush
    if (Tb >= 2) {
#pragma unroll
      for (int c = 0; c < kBandBtAhead; ++c) x[c] = fetch(Tb - 1 - kBandBtRows * c, s, d[c]);
      for (int t_hi = Tb - 1; t_hi >= 1; t_hi -= kBandBtRows * kBandBtAhead) {
#pragma unroll
        for (int c = 0; c < kBandBtAhead; ++c) {
          const int th = t_hi - kBandBtRows * c;
          if (th >= 1) {  // wave-uniform
            const uint32_t cur = x[c];
            const int dc = d[c];
            x[c] = fetch(th - kBandBtRows * kBandBtAhead, s, d[c]);   // kBandBtAhead chunks ahead of the walk (clamped past the start)
#pragma unroll
            for (int r = 0; r < kBandBtRows; ++r) {
              const int t = th - r;
              if (t >= 1) {  // wave-uniform
                mine = (lane == (t & 63)) ? s : mine;
                if ((t & 63) == 0 && t + lane < Tb) fs[t + lane] = mine;
                const int col = min(max(dc - (s >> 4), 0), kBandBtCols - 1);
                const uint32_t word = __builtin_amdgcn_readlane(cur, __builtin_amdgcn_readfirstlane(r * kBandBtCols + col));
                const int back = (int)((word >> (2 * (s & 15))) & 3u);
                s = max(s - back, 0);
              }
            }
          }
        }
      }
    }
    mine = (lane == 0) ? s : mine;                      // frame 0
    if (lane < Tb) fs[lane] = mine;
  }
  __syncthreads();

  // ------------------------------------------------------------------ frames and spans, in parallel over frames
  for (int t = threadIdx.x; t < (int)T; t += NT) {
    float e = 0.f;
    if (feasible && t < Tb) {
      const int st = fs[t];
      e = lp[(int64_t)t * C + ((st & 1) ? labs[st >> 1] : blank)];
      if (st & 1) {
        // an odd state that differs from the previous frame's opens label st >> 1; one that differs from the next closes it
        const int prev = t > 0 ? fs[t - 1] : -1;
        const int next = t + 1 < Tb ? fs[t + 1] : -1;
        if (prev != st) l_start[st >> 1] = t;
        if (next != st) l_end[st >> 1] = t + 1;
      }
    } else {
      fs[t] = -1;
    }
    if (t >= Tb) bl[t] = -1;
    flp[t] = e;
  }
}

// states per lane and waves for a band: NS = 16 on W / 1024 waves, else NS = 4 on W / 256; nw = 0: not a band this file takes
struct BandGeom {
  int ns, nw;
};
static inline BandGeom band_geom(int64_t band) {
  if (band < 256 || band % 256 != 0 || band > LASR_CTC_ALIGN_LONG_MAX_BAND) return {0, 0};
  if (band % 1024 == 0) return {16, (int)(band / 1024)};
  if (band / 256 <= kBandMaxWaves) return {4, (int)(band / 256)};
  return {0, 0};
}

}  // namespace lasr

using namespace lasr;

extern "C" int64_t lasr_ctc_align_long_period(void) { return kBandR; }
extern "C" int64_t lasr_ctc_align_long_granule(void) { return kBandG; }

extern "C" size_t lasr_ctc_align_long_workspace_bytes(int64_t B, int64_t T, int64_t S_max, int64_t band) {
  if (B <= 0 || T <= 0 || S_max < 0 || S_max > LASR_CTC_ALIGN_LONG_MAX_LABELS || band_geom(band).nw == 0) return 0;
  return align_up((size_t)B * (size_t)T * (size_t)(band / 4), 256);
}

extern "C" int lasr_ctc_align_long(const float* logp, const int64_t* targets, const int32_t* in_lens, const int32_t* tgt_lens, int64_t B,
                                   int64_t T, int64_t C, int64_t S_max, int blank, int64_t band, float* score, int32_t* frame_state,
                                   float* frame_logp, int32_t* label_start, int32_t* label_end, int32_t* status, int32_t* band_lo,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  LASR_CHECK_ARG(logp && tgt_lens && score && frame_state && frame_logp && status && band_lo && workspace,
                 "lasr_ctc_align_long: null pointer");
  LASR_CHECK_ARG(S_max <= 0 || (targets && label_start && label_end), "lasr_ctc_align_long: null pointer");
  LASR_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "lasr_ctc_align_long: the workspace must be 4-byte aligned");
  LASR_CHECK_SHAPE(B > 0 && B < ((int64_t)1 << 31) && T > 0 && T < ((int64_t)1 << 31) - 64 && C > 1 && C < ((int64_t)1 << 29) && blank >= 0 &&
                       blank < C,
                   "lasr_ctc_align_long: shape");
  LASR_CHECK_SHAPE(S_max >= 0 && S_max <= LASR_CTC_ALIGN_LONG_MAX_LABELS, "lasr_ctc_align_long: S_max=%lld outside [0, %d]", (long long)S_max,
                   LASR_CTC_ALIGN_LONG_MAX_LABELS);
  const BandGeom geo = band_geom(band);
  LASR_CHECK_SHAPE(geo.nw != 0, "lasr_ctc_align_long: band=%lld is not a multiple of 256 in [256, 4096] or of 1024 in [1024, %d]",
                   (long long)band, LASR_CTC_ALIGN_LONG_MAX_BAND);
  if (workspace_bytes < lasr_ctc_align_long_workspace_bytes(B, T, S_max, band)) return fail(LASR_E_WORKSPACE, "lasr_ctc_align_long: workspace");
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64u * (unsigned)geo.nw), 0, as_stream(stream), logp, targets, in_lens, tgt_lens, T, C,
                       S_max, blank, (int)band, score, frame_state, frame_logp, label_start, label_end, status, band_lo,
                       static_cast<uint32_t*>(workspace));
  };
  LASR_TRY(with_int<4, 16>(geo.ns, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    if (NS == 16 && geo.nw > 4) launch(ctc_align_long_kernel<16, true, true>);
    else with_bool(geo.nw > 1, [&](auto mw) { launch(ctc_align_long_kernel<NS, decltype(mw)::value, false>); });
  }));
  LASR_LAUNCH_CHECK("ctc_align_long_kernel");
  return 0;
}
