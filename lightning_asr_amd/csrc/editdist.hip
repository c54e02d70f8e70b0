// Levenshtein distance between the greedy-decoded hypotheses and the references, on the device, for a whole batch:
// the WER / CER numerator and denominator of utils/asr_metrics.py:26-59,187-228 without the per-step D2H of the
// token ids and the Python loop over utterances.
//
//   CER mode (space_id < 0; the reference's file-path vocabularies, train.py:216-219): units = token ids.
//   WER mode (space_id >= 0): units = words = maximal runs of non-space tokens (str.split() semantics: leading /
//   trailing / repeated spaces produce no empty word); a word is compared through a 64-bit polynomial hash of its ids.
//
// One wave per utterance.  Row i of the DP (hypothesis unit i against every reference prefix j):
//   cur[j] = min(prev[j] + 1, prev[j-1] + (a_i != b_j), cur[j-1] + 1)
// The last term is a running dependency along j; with t[j] = min(prev[j] + 1, prev[j-1] + cost) it unrolls to
//   cur[j] = j + min_{k <= j} (t[k] - k),
// a prefix-min, so a row is: elementwise t, one wave prefix-min scan (6 DPP/shuffle steps), add j.  The reference row
// lives in registers (NJ cells per lane), `prev` never leaves the wave.
//
// edit_align_kernel (further down) is the same DP with back-pointers and the canonical trace-back: which of the errors are
// substitutions, deletions and insertions (lasr_edit_align_batch; evaluation only, the training step does not launch it).
#include "common.h"
#include <algorithm>

namespace lasr {

static constexpr int kEdMaxUnits = 2048;          // units (tokens or words) per side
static constexpr int kEdNJ = kEdMaxUnits / 64;    // DP cells per lane

// sequence of DP units of one side -> LDS (u64), returns the count.  One lane walks the tokens (<= a few hundred).
__device__ __forceinline__ int ed_units(const int32_t* tok32, const int64_t* tok64, int n, int space_id, unsigned long long* s_u) {
  int cnt = 0;
  if (space_id < 0) {
    for (int i = 0; i < n && cnt < kEdMaxUnits; ++i) s_u[cnt++] = (unsigned long long)(tok32 ? (long long)tok32[i] : tok64[i]) + 1ull;
    return cnt;
  }
  unsigned long long h = 0ull;
  bool in_word = false;
  for (int i = 0; i < n; ++i) {
    const long long t = tok32 ? (long long)tok32[i] : tok64[i];
    if (t == space_id) {
      if (in_word && cnt < kEdMaxUnits) s_u[cnt++] = h;
      in_word = false; h = 0ull;
    } else {
      h = h * 1000003ull + (unsigned long long)(t + 1) * 0x9E3779B97F4A7C15ull + 0x7F4A7C15ull;   // order-sensitive
      in_word = true;
    }
  }
  if (in_word && cnt < kEdMaxUnits) s_u[cnt++] = h;
  return cnt;
}

// both sides of utterance b -> LDS units s_a (hypothesis) / s_b (reference) and their counts s_n[0] / s_n[1]; ends in a barrier
__device__ __forceinline__ void ed_stage_units(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_lens, int64_t ld_h,
                                               const int64_t* __restrict__ ref, const int32_t* __restrict__ ref_lens, int64_t ld_r,
                                               int space_id, int b, int lane, unsigned long long* s_a, unsigned long long* s_b, int* s_n) {
  const int nh = max(0, min(hyp_lens[b], (int)ld_h)), nr = max(0, min(ref_lens[b], (int)ld_r));
  if (space_id < 0) {             // CER: a unit is a token id, copied by the whole wave
    for (int i = lane; i < min(nh, kEdMaxUnits); i += 64) s_a[i] = (unsigned long long)(long long)hyp[(int64_t)b * ld_h + i] + 1ull;
    for (int i = lane; i < min(nr, kEdMaxUnits); i += 64) s_b[i] = (unsigned long long)ref[(int64_t)b * ld_r + i] + 1ull;
    if (lane == 0) { s_n[0] = min(nh, kEdMaxUnits); s_n[1] = min(nr, kEdMaxUnits); }
  } else if (lane == 0) {         // WER: one lane cuts the token stream into words (a few hundred tokens)
    s_n[0] = ed_units(hyp + (int64_t)b * ld_h, nullptr, nh, space_id, s_a);
    s_n[1] = ed_units(nullptr, ref + (int64_t)b * ld_r, nr, space_id, s_b);
  }
  __syncthreads();
}

__device__ __forceinline__ int wave_prefix_min_excl_carry(int v, int lane) {   // inclusive prefix-min over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v = min(v, o);
  }
  return v;
}

// grid = B, block = 64.  hyp [B][ld_h] i32 with hyp_lens; ref [B][ld_r] i64 with ref_lens (i32).
// NJ = DP cells per lane: 64 * NJ >= the longer of (hypothesis, reference) pitch of the batch (a row costs NJ cell updates per lane
// whatever the actual length: 2048 cells per row for every batch cost 77 us at cfg2)
// dist[b] = Levenshtein(hyp units, ref units), ref_units[b] = number of reference units.
template <int NJ>
__global__ __launch_bounds__(64) void edit_distance_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_lens, int64_t ld_h,
                                                           const int64_t* __restrict__ ref, const int32_t* __restrict__ ref_lens, int64_t ld_r,
                                                           int space_id, int32_t* __restrict__ dist, int32_t* __restrict__ ref_units) {
  __shared__ unsigned long long s_a[kEdMaxUnits], s_b[kEdMaxUnits];
  __shared__ int s_n[2];
  const int b = blockIdx.x, lane = threadIdx.x;
  ed_stage_units(hyp, hyp_lens, ld_h, ref, ref_lens, ld_r, space_id, b, lane, s_a, s_b, s_n);
  // The distance is symmetric: the LONGER sequence goes onto the lanes (the row cost does not depend on it), the loop runs over the
  // SHORTER one - an untrained model's greedy output is ~T' tokens against a 100-label reference: 501 dependent rows became 100.
  const int n_ref = s_n[1];
  const bool swap = s_n[0] > s_n[1];                       // wave-uniform
  const unsigned long long* s_rows = swap ? s_b : s_a;
  const unsigned long long* s_cols = swap ? s_a : s_b;
  const int na = swap ? s_n[1] : s_n[0], nb = swap ? s_n[0] : s_n[1];
  // lane owns column positions j = lane*NJ + q + 1 (q < NJ): contiguous per lane, so the in-lane part of the scan is serial
  unsigned long long bj[NJ];
  int prev[NJ];                // prev[q] = D[i-1][j]
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    const int j = lane * NJ + q + 1;
    bj[q] = j <= nb ? s_cols[j - 1] : 0ull;
    prev[q] = j;                  // D[0][j] = j
  }
  for (int i = 1; i <= na; ++i) {
    const unsigned long long ai = s_rows[i - 1];
    // D[i-1][j-1] for this lane's first cell comes from the previous lane's last cell (lane 0: D[i-1][0] = i-1)
    int left_prev = __shfl_up(prev[NJ - 1], 1, 64);
    if (lane == 0) left_prev = i - 1;
    int t[NJ];
    int run = 0x3fffffff;         // min over this lane's cells of t[k] - k
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      const int j = lane * NJ + q + 1;
      const int diag = q == 0 ? left_prev : prev[q - 1];
      const int v = min(prev[q] + 1, diag + (ai != bj[q] ? 1 : 0));
      run = min(run, v - j);
      t[q] = run;                 // in-lane prefix of (t - k)
    }
    // exclusive prefix-min over the lanes before this one, seeded with the column-0 term D[i][0] - 0 = i
    int incl = wave_prefix_min_excl_carry(run, lane);
    int before = __shfl_up(incl, 1, 64);
    if (lane == 0) before = 0x3fffffff;
    before = min(before, i);      // cur[0] = i contributes (i - 0) to every j
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      const int j = lane * NJ + q + 1;
      prev[q] = j + min(t[q], before);
    }
  }
  // D[na][nb]: nb = 0 -> na
  int res = na;
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    const int j = lane * NJ + q + 1;
    if (j == nb) res = prev[q];
  }
  const int owner = nb > 0 ? (nb - 1) / NJ : 0;
  res = __shfl(res, owner, 64);
  if (lane == 0) { dist[b] = res; ref_units[b] = n_ref; }
}

// totals[0] += sum dist, totals[1] += sum ref_units  (the Metric's `scores` / `words` states, utils/asr_metrics.py:114-115)
__global__ __launch_bounds__(64) void edit_totals_kernel(const int32_t* __restrict__ dist, const int32_t* __restrict__ ref_units, int64_t B,
                                                         long long* __restrict__ totals) {
  long long s = 0, w = 0;
  for (int64_t i = threadIdx.x; i < B; i += 64) { s += dist[i]; w += ref_units[i]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); w += __shfl_xor(w, o, 64); }
  if (threadIdx.x == 0) { totals[0] += s; totals[1] += w; }
}

// ---- the alignment behind the distance: hits / substitutions / deletions / insertions (lasr_edit_align_batch) ------------------
// edit_distance_kernel's DP with one addition: after a row's scan every cell knows its three predecessors, so it emits a 2-bit
// back-pointer; a lane's NJ <= 32 pointers are one u64 word, a row is 64 words (one coalesced 512 B store), an utterance's table
// is bp[row][lane] with row < min(units per side).  The canonical walk (include/lasr.h) prefers the diagonal, then the deletion,
// then the insertion.  In DP terms a deletion is the move that drops a reference unit: "left" while the reference sits on the
// lanes, "up" once the sides are swapped - the tie-break flips with the orientation, the script does not.
//   pointer codes: 0 diagonal with equal units (hit), 3 diagonal with different units (substitution), 1 left, 2 up
static constexpr int kEaGroup = 8;                // DP rows the trace-back requests at once
static constexpr int kEaPad = 255;                // LASR_EDIT_PAD: ops past n_ops

template <int NJ>
__device__ __forceinline__ int ea_pointer(unsigned lo, unsigned hi, int j) {    // pointer of column j >= 1 of the row held in (lo, hi)
  const int c = j - 1, owner = c / NJ, sh = (c % NJ) * 2;
  if (NJ <= 16) return (int)(((unsigned)__builtin_amdgcn_readlane((int)lo, owner) >> sh) & 3u);
  const unsigned x = (sh & 32) ? (unsigned)__builtin_amdgcn_readlane((int)hi, owner) : (unsigned)__builtin_amdgcn_readlane((int)lo, owner);
  return (int)((x >> (sh & 31)) & 3u);
}

// grid = B, block = 64; bp: B * bp_rows * 64 words.  counts [B][4] = hits, subs, dels, ins; ops [B][ld_ops] u8 forward script,
// kEaPad past n_ops[b]; confusion (token mode, may be null): (n_classes + 1)^2 i32, row = reference label, column = hypothesis label,
// index n_classes = none.
template <int NJ>
__global__ __launch_bounds__(64) void edit_align_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_lens, int64_t ld_h,
                                                        const int64_t* __restrict__ ref, const int32_t* __restrict__ ref_lens, int64_t ld_r,
                                                        int space_id, int32_t* __restrict__ dist, int32_t* __restrict__ ref_units,
                                                        int32_t* __restrict__ counts, uint8_t* __restrict__ ops, int64_t ld_ops,
                                                        int32_t* __restrict__ n_ops, int32_t* confusion, int n_classes,
                                                        unsigned long long* bp_all, int64_t bp_rows) {
  __shared__ unsigned long long s_a[kEdMaxUnits], s_b[kEdMaxUnits];
  __shared__ uint8_t s_ops[2 * kEdMaxUnits];      // the script as the walk produces it: backwards
  __shared__ int s_n[2];
  const int b = blockIdx.x, lane = threadIdx.x;
  ed_stage_units(hyp, hyp_lens, ld_h, ref, ref_lens, ld_r, space_id, b, lane, s_a, s_b, s_n);
  const int n_hyp = __builtin_amdgcn_readfirstlane(s_n[0]), n_ref = __builtin_amdgcn_readfirstlane(s_n[1]);
  const bool swap = n_hyp > n_ref;                         // as edit_distance_kernel: the longer side on the lanes
  const unsigned long long* s_rows = swap ? s_b : s_a;
  const unsigned long long* s_cols = swap ? s_a : s_b;
  const int na = swap ? n_ref : n_hyp, nb = swap ? n_hyp : n_ref;
  unsigned long long* bp = bp_all + (int64_t)b * bp_rows * 64 + lane;       // this lane's word of row i: bp[(i - 1) * 64]
  unsigned long long bj[NJ];
  int prev[NJ];
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    const int j = lane * NJ + q + 1;
    bj[q] = j <= nb ? s_cols[j - 1] : 0ull;
    prev[q] = j;
  }
  for (int i = 1; i <= na; ++i) {
    const unsigned long long ai = s_rows[i - 1];
    int left_prev = __shfl_up(prev[NJ - 1], 1, 64);
    if (lane == 0) left_prev = i - 1;
    int t[NJ];
    int run = 0x3fffffff;
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      const int j = lane * NJ + q + 1;
      const int diag = q == 0 ? left_prev : prev[q - 1];
      const int v = min(prev[q] + 1, diag + (ai != bj[q] ? 1 : 0));
      run = min(run, v - j);
      t[q] = run;
    }
    int incl = wave_prefix_min_excl_carry(run, lane);
    int before = __shfl_up(incl, 1, 64);
    if (lane == 0) before = 0x3fffffff;
    before = min(before, i);
    // D[i][j-1] of this lane's first cell is the previous lane's last cell of THIS row: known only now (lane 0: D[i][0] = i)
    int left_cur = __shfl_up(lane * NJ + NJ + min(t[NJ - 1], before), 1, 64);
    if (lane == 0) left_cur = i;
    unsigned long long word = 0ull;
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      const int j = lane * NJ + q + 1;
      const int cur = j + min(t[q], before);
      const int diag = q == 0 ? left_prev : prev[q - 1];      // prev[q - 1] is still row i-1: it is overwritten one step later
      const int sub = ai != bj[q] ? 1 : 0;
      const bool diag_ok = diag + sub == cur, up_ok = prev[q] + 1 == cur, left_ok = left_cur + 1 == cur;
      const int other = swap ? (up_ok ? 2 : 1) : (left_ok ? 1 : 2);      // the deletion before the insertion, in either orientation
      word |= (unsigned long long)(diag_ok ? (sub ? 3 : 0) : other) << (2 * q);
      if (q > 0) prev[q - 1] = left_cur;
      left_cur = cur;
    }
    prev[NJ - 1] = left_cur;
    bp[(int64_t)(i - 1) * 64] = word;
  }
  int res = na;
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    const int j = lane * NJ + q + 1;
    if (j == nb) res = prev[q];
  }
  res = __shfl(res, nb > 0 ? (nb - 1) / NJ : 0, 64);

  // ---- trace-back, wave-uniform: every lane keeps its word of kEaGroup rows in registers (coalesced loads, the next group already
  // requested while this one is walked); a step inside a row is a readlane and a shift, a diagonal or up move goes on to the next
  // register.  Each lane reads back only the words it wrote itself.
  const int left_op = swap ? 3 : 2, up_op = swap ? 2 : 3;
  int i = na, j = nb, n = 0;
  auto emit = [&](int op) {
    if (lane == 0) s_ops[n] = (uint8_t)op;
    ++n;
  };
  auto load_row = [&](int row) -> unsigned long long { return row >= 1 ? bp[(int64_t)(row - 1) * 64] : 0ull; };
  unsigned long long g[kEaGroup], g_next[kEaGroup];
#pragma unroll
  for (int r = 0; r < kEaGroup; ++r) g[r] = load_row(i - r);
  while (i > 0) {
#pragma unroll
    for (int r = 0; r < kEaGroup; ++r) g_next[r] = load_row(i - kEaGroup - r);
#pragma unroll
    for (int r = 0; r < kEaGroup; ++r) {
      if (i > 0) {                                           // g[r] is row i: each r leaves exactly one row behind
        const unsigned lo = (unsigned)g[r], hi = (unsigned)(g[r] >> 32);
        for (;;) {
          const int mv = j > 0 ? ea_pointer<NJ>(lo, hi, j) : 2;
          if (mv == 1) { emit(left_op); --j; continue; }
          if (mv == 2) emit(up_op);
          else { emit(mv == 0 ? 0 : 1); --j; }
          --i;
          break;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kEaGroup; ++r) g[r] = g_next[r];
  }
  for (int k = lane; k < j; k += 64) s_ops[n + k] = (uint8_t)left_op;       // row 0: only left moves remain
  n += j;
  __syncthreads();

  // ---- forward script, counts, confusion: 64 ops per pass; an op's unit positions are prefix counts of the ops before it
  uint8_t* out = ops + (int64_t)b * ld_ops;
  int c_hit = 0, c_sub = 0, c_del = 0, c_ins = 0;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    const int op = k < n ? s_ops[n - 1 - k] : kEaPad;
    if (k < n) out[k] = (uint8_t)op;
    const unsigned long long m_hit = __ballot(op == 0), m_sub = __ballot(op == 1), m_del = __ballot(op == 2), m_ins = __ballot(op == 3);
    if (confusion) {
      const unsigned long long below = (1ull << lane) - 1ull;
      const int ih = c_hit + c_sub + c_ins + __popcll((m_hit | m_sub | m_ins) & below);
      const int ir = c_hit + c_sub + c_del + __popcll((m_hit | m_sub | m_del) & below);
      if (k < n) {
        const long long none = n_classes;
        const long long lh = op == 2 ? none : (long long)s_a[ih] - 1, lr = op == 3 ? none : (long long)s_b[ir] - 1;
        if (lh >= 0 && lh <= none && lr >= 0 && lr <= none && (op == 2 || lh < none) && (op == 3 || lr < none))
          atomicAdd(confusion + lr * (none + 1) + lh, 1);
      }
    }
    c_hit += __popcll(m_hit); c_sub += __popcll(m_sub); c_del += __popcll(m_del); c_ins += __popcll(m_ins);
  }
  for (int64_t k = n + lane; k < ld_ops; k += 64) out[k] = (uint8_t)kEaPad;
  if (lane == 0) {
    dist[b] = res; ref_units[b] = n_ref; n_ops[b] = n;
    counts[4 * b] = c_hit; counts[4 * b + 1] = c_sub; counts[4 * b + 2] = c_del; counts[4 * b + 3] = c_ins;
  }
}

// totals[0..5] += sums of dist, ref_units, hits, subs, dels, ins
__global__ __launch_bounds__(64) void edit_align_totals_kernel(const int32_t* __restrict__ dist, const int32_t* __restrict__ ref_units,
                                                               const int32_t* __restrict__ counts, int64_t B, long long* __restrict__ totals) {
  long long s[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = threadIdx.x; i < B; i += 64) {
    s[0] += dist[i]; s[1] += ref_units[i];
#pragma unroll
    for (int c = 0; c < 4; ++c) s[2 + c] += counts[4 * i + c];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[c] += __shfl_xor(s[c], o, 64);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 6; ++c) totals[c] += s[c];
  }
}

// one training step's logged scalars folded into device accumulators (no D2H per step)
__global__ __launch_bounds__(64) void step_metrics_kernel(const float* __restrict__ loss, const int32_t* __restrict__ dist,
                                                          const int32_t* __restrict__ ref_units, int64_t B, double* __restrict__ acc) {
  long long s = 0, w = 0;
  for (int64_t i = threadIdx.x; i < B; i += 64) { s += dist[i]; w += ref_units[i]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); w += __shfl_xor(w, o, 64); }
  if (threadIdx.x == 0) {
    const double wer = w != 0 ? (double)s / (double)w : (double)INFINITY;    // utils/asr_metrics.py:59 (inf when no reference units)
    const double l = (double)loss[0];
    acc[0] += l; acc[1] += wer; acc[2] += 1.0; acc[3] = l; acc[4] = wer; acc[5] += (double)s; acc[6] += (double)w;
  }
}

}  // namespace lasr

using namespace lasr;

extern "C" int lasr_step_metrics(const float* loss, const int32_t* dist, const int32_t* ref_units, int64_t B, double* acc, void* stream) {
  LASR_CHECK_ARG(loss && dist && ref_units && acc && B > 0, "lasr_step_metrics: bad argument");
  hipLaunchKernelGGL(step_metrics_kernel, dim3(1), dim3(64), 0, as_stream(stream), loss, dist, ref_units, B, acc);
  LASR_LAUNCH_CHECK("step_metrics_kernel");
  return 0;
}

extern "C" int lasr_edit_distance_batch(const int32_t* hyp_tokens, const int32_t* hyp_lens, int64_t ld_hyp, const int64_t* ref_tokens,
                                        const int32_t* ref_lens, int64_t ld_ref, int64_t B, int space_id, int32_t* dist, int32_t* ref_units,
                                        int64_t* totals, void* stream) {
  LASR_CHECK_ARG(hyp_tokens && hyp_lens && ref_tokens && ref_lens && dist && ref_units, "lasr_edit_distance_batch: null pointer");
  LASR_CHECK_SHAPE(B > 0 && B < (1 << 20) && ld_hyp > 0 && ld_ref > 0, "lasr_edit_distance_batch: B=%lld", (long long)B);
  LASR_CHECK_SHAPE(ld_hyp <= kEdMaxUnits && ld_ref <= kEdMaxUnits, "lasr_edit_distance_batch: more than %d tokens per utterance",
                   kEdMaxUnits);
  hipStream_t st = as_stream(stream);
  const int64_t ld_cols = std::max(ld_hyp, ld_ref);        // either side may end up on the lanes
  if (ld_cols <= 128)
    hipLaunchKernelGGL(edit_distance_kernel<2>, dim3((unsigned)B), dim3(64), 0, st, hyp_tokens, hyp_lens, ld_hyp, ref_tokens, ref_lens, ld_ref,
                       space_id, dist, ref_units);
  else if (ld_cols <= 512)
    hipLaunchKernelGGL(edit_distance_kernel<8>, dim3((unsigned)B), dim3(64), 0, st, hyp_tokens, hyp_lens, ld_hyp, ref_tokens, ref_lens, ld_ref,
                       space_id, dist, ref_units);
  else
    hipLaunchKernelGGL(edit_distance_kernel<kEdNJ>, dim3((unsigned)B), dim3(64), 0, st, hyp_tokens, hyp_lens, ld_hyp, ref_tokens, ref_lens, ld_ref,
                       space_id, dist, ref_units);
  LASR_LAUNCH_CHECK("edit_distance_kernel");
  if (totals) {
    hipLaunchKernelGGL(edit_totals_kernel, dim3(1), dim3(64), 0, st, dist, ref_units, B, reinterpret_cast<long long*>(totals));
    LASR_LAUNCH_CHECK("edit_totals_kernel");
  }
  return 0;
}

extern "C" size_t lasr_edit_align_workspace_bytes(int64_t B, int64_t ld_hyp, int64_t ld_ref) {
  if (B <= 0 || ld_hyp <= 0 || ld_ref <= 0) return 0;
  return align_up((size_t)B * (size_t)std::min(ld_hyp, ld_ref) * 64 * sizeof(unsigned long long), 256);     // bp[B][rows][64]
}

extern "C" int lasr_edit_align_batch(const int32_t* hyp_tokens, const int32_t* hyp_lens, int64_t ld_hyp, const int64_t* ref_tokens,
                                     const int32_t* ref_lens, int64_t ld_ref, int64_t B, int space_id, int32_t* dist, int32_t* ref_units,
                                     int32_t* counts, uint8_t* ops, int64_t ld_ops, int32_t* n_ops, int64_t* totals, int32_t* confusion,
                                     int n_classes, void* workspace, size_t workspace_bytes, void* stream) {
  LASR_CHECK_ARG(hyp_tokens && hyp_lens && ref_tokens && ref_lens && dist && ref_units && counts && ops && n_ops && workspace,
                 "lasr_edit_align_batch: null pointer");
  LASR_CHECK_ARG(!confusion || space_id < 0, "lasr_edit_align_batch: the confusion matrix is over token ids: not with space_id >= 0");
  LASR_CHECK_ARG(!confusion || (n_classes > 0 && n_classes < (1 << 20)), "lasr_edit_align_batch: n_classes=%d", n_classes);
  LASR_CHECK_SHAPE(B > 0 && B < (1 << 20) && ld_hyp > 0 && ld_ref > 0, "lasr_edit_align_batch: B=%lld", (long long)B);
  LASR_CHECK_SHAPE(ld_hyp <= kEdMaxUnits && ld_ref <= kEdMaxUnits, "lasr_edit_align_batch: more than %d tokens per utterance", kEdMaxUnits);
  LASR_CHECK_SHAPE(ld_ops >= ld_hyp + ld_ref, "lasr_edit_align_batch: ld_ops=%lld is shorter than ld_hyp + ld_ref = %lld", (long long)ld_ops,
                   (long long)(ld_hyp + ld_ref));
  if (workspace_bytes < lasr_edit_align_workspace_bytes(B, ld_hyp, ld_ref)) return fail(LASR_E_WORKSPACE, "lasr_edit_align_batch: workspace");
  hipStream_t st = as_stream(stream);
  const int64_t ld_cols = std::max(ld_hyp, ld_ref), bp_rows = std::min(ld_hyp, ld_ref);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64), 0, st, hyp_tokens, hyp_lens, ld_hyp, ref_tokens, ref_lens, ld_ref, space_id, dist,
                       ref_units, counts, ops, ld_ops, n_ops, confusion, n_classes, static_cast<unsigned long long*>(workspace), bp_rows);
  };
  if (ld_cols <= 128) launch(edit_align_kernel<2>);             // the thresholds of lasr_edit_distance_batch
  else if (ld_cols <= 512) launch(edit_align_kernel<8>);
  else launch(edit_align_kernel<kEdNJ>);
  LASR_LAUNCH_CHECK("edit_align_kernel");
  if (totals) {
    hipLaunchKernelGGL(edit_align_totals_kernel, dim3(1), dim3(64), 0, st, dist, ref_units, counts, B, reinterpret_cast<long long*>(totals));
    LASR_LAUNCH_CHECK("edit_align_totals_kernel");
  }
  return 0;
}
