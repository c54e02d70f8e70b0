// Greedy CTC decode with confidences, from the log-probs, on the device (include/lasr.h, lasr_greedy_confidence).
// Replaces the reference's host loop over frames (ssl_codec/utils.py:8-66 on a (T', C) copy of every utterance's log-probs):
// the (B, T, C) block is read once, and nothing larger than (B, T) is written.
//
// Two launches on the caller's stream, no communication between workgroups inside a launch:
//  1. row statistics: m_t = max_c logp[b][t][c] and a_t = the lowest class attaining it, for every frame t < Tb, into the
//     workspace ([B*T] f32, then [B*T] i32).  This pass moves all the bytes, so it is laid over the whole chip: one row per
//     wave.  Rows of more than kGreedyConfNarrowC classes are read 16 bytes per lane, with a scalar head up to the row's first
//     16-byte boundary and a scalar tail (a row of 4334 floats starts 8-byte aligned, one of an odd C 4-byte aligned); narrower
//     rows share a wave, 64 / G rows of G = 2^ceil(log2 C) lanes each, four such groups in flight per wave.
//  2. collapse: one workgroup per utterance walks its (m, a) in tiles of kGreedyConfTile frames.  Within a tile one segmented
//     inclusive scan (segments = runs of equal argmax; value = f64 sum, f32 min, frame count) and one plain scan (emitting
//     frames) run over the wave by shuffles and over the four waves through LDS; the open run and the token count are carried
//     to the next tile.  A token is written by the LAST frame of its run, which then holds the run's sum, min, length and the
//     token's index, so a run that straddles tiles needs nothing more than the carry.
#include "common.h"

#include <math.h>

namespace lasr {

static constexpr int kGreedyConfNarrowC = 64;     // up to here a row is a power-of-two group of lanes, above it a whole wave
static constexpr int kGreedyConfTile = 256;       // frames per tile of the collapse = threads of its workgroup
static constexpr int kGreedyConfNarrowGroups = 4; // row groups a wave of the narrow form keeps in flight
static constexpr int kNoClass = 0x7fffffff;
static constexpr float kNegInf = -INFINITY;

__device__ __forceinline__ int greedy_conf_len(const int32_t* __restrict__ lens, int64_t b, int64_t T) {
  return lens ? (int)min((int64_t)max(lens[b], 0), T) : (int)T;
}

__device__ __forceinline__ void take_max(float v, int c, float& m, int& mi) {
  if (v > m) { m = v; mi = c; }              // classes arrive in ascending order within a lane: the first of equals stays
}

// ---- pass 1, wide rows: one wave per row --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void greedy_conf_rows_wide_kernel(const float* __restrict__ logp, const int32_t* __restrict__ lens,
                                                                    int64_t N, int64_t T, int64_t C, float* __restrict__ row_max,
                                                                    int32_t* __restrict__ row_arg) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int64_t b = row / T;
  if (row - b * T >= greedy_conf_len(lens, b, T)) return;      // padding frames are never read
  const float* x = logp + row * C;
  const int head = (int)min((int64_t)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 2), C);
  const int64_t nvec = (C - head) >> 2;
  const int tail = (int)(C - head - nvec * 4);
  const float4* xv = reinterpret_cast<const float4*>(x + head);
  float m = kNegInf;
  int mi = kNoClass;
  if (lane < head) take_max(x[lane], lane, m, mi);
  int64_t v = lane;
  for (; v + 192 < nvec; v += 256) {                            // four 16-byte loads in flight per lane
    const float4 q0 = xv[v], q1 = xv[v + 64], q2 = xv[v + 128], q3 = xv[v + 192];
    const float4 q[4] = {q0, q1, q2, q3};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = head + (int)(v + 64 * j) * 4;
      take_max(q[j].x, c, m, mi); take_max(q[j].y, c + 1, m, mi); take_max(q[j].z, c + 2, m, mi); take_max(q[j].w, c + 3, m, mi);
    }
  }
  for (; v < nvec; v += 64) {
    const float4 q = xv[v];
    const int c = head + (int)v * 4;
    take_max(q.x, c, m, mi); take_max(q.y, c + 1, m, mi); take_max(q.z, c + 2, m, mi); take_max(q.w, c + 3, m, mi);
  }
  if (lane < tail) {
    const int c = head + (int)nvec * 4 + lane;
    take_max(x[c], c, m, mi);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  if (lane == 0) {
    row_max[row] = m;
    row_arg[row] = mi == kNoClass ? 0 : mi;                     // a row of -inf only: class 0
  }
}

// ---- pass 1, narrow rows (C <= 64): G = 2^ceil(log2 C) lanes per row, 64 / G rows per wave instruction -------------------------
__global__ __launch_bounds__(256) void greedy_conf_rows_narrow_kernel(const float* __restrict__ logp, const int32_t* __restrict__ lens,
                                                                      int64_t N, int64_t T, int C, int G, float* __restrict__ row_max,
                                                                      int32_t* __restrict__ row_arg) {
  const int lane = threadIdx.x & 63;
  const int per = 64 / G;                                        // rows per group
  const int sub = lane / G, c = lane - sub * G;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row0 = wave * (per * kGreedyConfNarrowGroups) + sub;
  float m[kGreedyConfNarrowGroups];
  bool live[kGreedyConfNarrowGroups];
#pragma unroll
  for (int k = 0; k < kGreedyConfNarrowGroups; ++k) {
    const int64_t row = row0 + (int64_t)k * per;
    live[k] = false;
    if (row < N) {
      const int64_t b = row / T;
      live[k] = row - b * T < greedy_conf_len(lens, b, T);
    }
    m[k] = live[k] && c < C ? logp[row * C + c] : kNegInf;
  }
#pragma unroll
  for (int k = 0; k < kGreedyConfNarrowGroups; ++k) {
    float mk = m[k];
    int mi = mk > kNegInf ? c : kNoClass;
    for (int o = G >> 1; o > 0; o >>= 1) {                       // stays inside the row's G lanes
      const float om = __shfl_xor(mk, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (om > mk || (om == mk && oi < mi)) { mk = om; mi = oi; }
    }
    if (live[k] && c == 0) {
      const int64_t row = row0 + (int64_t)k * per;
      row_max[row] = mk;
      row_arg[row] = mi == kNoClass ? 0 : mi;
    }
  }
}

// ---- pass 2: collapse, spans and confidences of one utterance ------------------------------------------------------------------
struct GreedyRun {        // the scanned value: the run that ends at (or passes through) a frame, and the emitting frames so far
  double sum;
  float mn;
  int cnt;
  int head;               // a run starts at or before this element, inside the scanned range
  int emits;
};

__device__ __forceinline__ void greedy_run_append(GreedyRun& left, const GreedyRun& right) {    // left = left (+) right
  if (right.head) {
    left.sum = right.sum; left.mn = right.mn; left.cnt = right.cnt; left.head = 1;
  } else {
    left.sum += right.sum; left.mn = fminf(left.mn, right.mn); left.cnt += right.cnt;
  }
  left.emits += right.emits;
}

struct GreedyFrame { float m; int a, prev, next; };

__device__ __forceinline__ GreedyFrame greedy_conf_frame(const float* __restrict__ m, const int32_t* __restrict__ a, int64_t t, int Tb) {
  GreedyFrame f;
  const bool in = t < Tb;
  f.m = in ? m[t] : 0.f;
  f.a = in ? a[t] : -1;
  f.prev = in && t > 0 ? a[t - 1] : -1;
  f.next = t + 1 < Tb ? a[t + 1] : -1;
  return f;
}

__global__ __launch_bounds__(kGreedyConfTile) void greedy_conf_collapse_kernel(
    const float* __restrict__ row_max, const int32_t* __restrict__ row_arg, const int32_t* __restrict__ lens, int64_t T, int blank,
    int32_t* __restrict__ tokens, int32_t* __restrict__ n_tokens, int32_t* __restrict__ tok_start, int32_t* __restrict__ tok_end,
    float* __restrict__ tok_mean, float* __restrict__ tok_min, double* __restrict__ utt_sum, int32_t* __restrict__ n_nonblank,
    float* __restrict__ conf) {
  constexpr int NW = kGreedyConfTile / 64;
  __shared__ GreedyRun s_agg[NW];
  __shared__ double s_sum[NW][2];
  __shared__ int s_nb[NW];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int Tb = greedy_conf_len(lens, b, T);
  const float* m = row_max + b * T;
  const int32_t* a = row_arg + b * T;
  int32_t* o_tok = tokens + b * T;
  int32_t* o_start = tok_start + b * T;
  int32_t* o_end = tok_end + b * T;
  float* o_mean = tok_mean + b * T;
  float* o_min = tok_min + b * T;

  GreedyRun carry = {0.0, INFINITY, 0, 0, 0};      // the run open at the end of the previous tile; emits = tokens so far
  double s_all = 0.0, s_lab = 0.0;
  int n_lab = 0;
  GreedyFrame nxt = greedy_conf_frame(m, a, tid, Tb);
  for (int64_t t0 = 0; t0 < Tb; t0 += kGreedyConfTile) {
    const int64_t t = t0 + tid;
    const GreedyFrame f = nxt;
    if (t0 + kGreedyConfTile < Tb) nxt = greedy_conf_frame(m, a, t + kGreedyConfTile, Tb);    // the next tile's loads fly during this one's scan
    const bool in = t < Tb;
    const bool head = !in || t == 0 || f.a != f.prev;           // frames past Tb are runs of their own: they close the last real run
    const bool last = in && (t + 1 >= Tb || f.next != f.a);
    const bool label = in && f.a != blank;
    if (in) s_all += (double)f.m;
    if (label) { s_lab += (double)f.m; ++n_lab; }

    GreedyRun r = {(double)f.m, f.m, 1, head ? 1 : 0, head && label ? 1 : 0};
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      GreedyRun l;
      l.sum = __shfl_up(r.sum, o, 64); l.mn = __shfl_up(r.mn, o, 64); l.cnt = __shfl_up(r.cnt, o, 64);
      l.head = __shfl_up(r.head, o, 64); l.emits = __shfl_up(r.emits, o, 64);
      if (lane >= o) { greedy_run_append(l, r); r = l; }
    }
    if (lane == 63) s_agg[wv] = r;
    __syncthreads();
    GreedyRun pre = carry;                                      // everything before this wave; then, before the next tile
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      if (j == wv) { GreedyRun mine = pre; greedy_run_append(mine, r); r = mine; }
      greedy_run_append(pre, s_agg[j]);
    }
    carry = pre;
    __syncthreads();                                            // s_agg is rewritten by the next tile

    if (last && label) {
      const int i = r.emits - 1;                                // the run's emitting frame is the last one counted
      o_tok[i] = f.a;
      o_start[i] = (int32_t)(t + 1 - r.cnt);
      o_end[i] = (int32_t)(t + 1);
      o_min[i] = r.mn;
      o_mean[i] = (float)(r.sum / (double)r.cnt);
    }
  }
  const int n = carry.emits;
  for (int64_t i = n + tid; i < T; i += kGreedyConfTile) {
    o_tok[i] = -1; o_start[i] = -1; o_end[i] = -1; o_min[i] = 0.f; o_mean[i] = 0.f;
  }
  s_all = wave_sum_d(s_all);
  s_lab = wave_sum_d(s_lab);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_lab += __shfl_xor(n_lab, o, 64);
  if (lane == 0) { s_sum[wv][0] = s_all; s_sum[wv][1] = s_lab; s_nb[wv] = n_lab; }
  __syncthreads();
  if (tid == 0) {
    double u0 = 0.0, u1 = 0.0;
    int nb = 0;
    for (int j = 0; j < NW; ++j) { u0 += s_sum[j][0]; u1 += s_sum[j][1]; nb += s_nb[j]; }
    n_tokens[b] = n;
    n_nonblank[b] = nb;
    utt_sum[b * 2] = u0;
    utt_sum[b * 2 + 1] = u1;
    conf[b * 2] = (float)(-(-1e-5 + u0) / ((double)Tb + 1e-6));
    conf[b * 2 + 1] = (float)(-(-1e-5 + u1) / ((double)nb + 1e-6));
  }
}

static bool greedy_conf_shape_ok(int64_t B, int64_t T, int64_t C) {
  return B >= 1 && T >= 1 && C >= 1 && B <= (((int64_t)1 << 31) - 1) / T && C < ((int64_t)1 << 31);
}

}  // namespace lasr

using namespace lasr;

extern "C" int64_t lasr_greedy_confidence_frame_tile(void) { return kGreedyConfTile; }
extern "C" int64_t lasr_greedy_confidence_narrow_classes(void) { return kGreedyConfNarrowC; }

extern "C" size_t lasr_greedy_confidence_workspace_bytes(int64_t B, int64_t T, int64_t C) {
  if (!greedy_conf_shape_ok(B, T, C)) return 0;
  return (size_t)(B * T) * (sizeof(float) + sizeof(int32_t));
}

extern "C" int lasr_greedy_confidence(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank,
                                      int32_t* tokens, int32_t* n_tokens, int32_t* tok_start, int32_t* tok_end, float* tok_mean,
                                      float* tok_min, double* utt_sum, int32_t* n_nonblank, float* conf, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  LASR_CHECK_ARG(logp && tokens && n_tokens && tok_start && tok_end && tok_mean && tok_min && utt_sum && n_nonblank && conf && workspace,
                 "lasr_greedy_confidence: null pointer");
  LASR_CHECK_SHAPE(greedy_conf_shape_ok(B, T, C), "lasr_greedy_confidence: B, T, C must be >= 1 and B*T below 2^31 (B=%lld T=%lld C=%lld)",
                   (long long)B, (long long)T, (long long)C);
  LASR_CHECK_SHAPE(blank >= 0 && blank < C, "lasr_greedy_confidence: blank %d outside [0, %lld)", blank, (long long)C);
  if (workspace_bytes < lasr_greedy_confidence_workspace_bytes(B, T, C))
    return fail(LASR_E_WORKSPACE, "lasr_greedy_confidence: workspace of %zu bytes, %zu needed", workspace_bytes,
                lasr_greedy_confidence_workspace_bytes(B, T, C));
  const int64_t N = B * T;
  float* row_max = static_cast<float*>(workspace);
  int32_t* row_arg = reinterpret_cast<int32_t*>(row_max + N);
  hipStream_t st = as_stream(stream);
  if (C > kGreedyConfNarrowC) {
    hipLaunchKernelGGL(greedy_conf_rows_wide_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, st, logp, lens, N, T, C, row_max, row_arg);
    LASR_LAUNCH_CHECK("greedy_conf_rows_wide_kernel");
  } else {
    int G = 1;
    while (G < C) G <<= 1;
    const int64_t rows_per_wave = (int64_t)(64 / G) * kGreedyConfNarrowGroups;
    hipLaunchKernelGGL(greedy_conf_rows_narrow_kernel, dim3((unsigned)cdiv(N, rows_per_wave * 4)), dim3(256), 0, st, logp, lens, N, T, (int)C,
                       G, row_max, row_arg);
    LASR_LAUNCH_CHECK("greedy_conf_rows_narrow_kernel");
  }
  hipLaunchKernelGGL(greedy_conf_collapse_kernel, dim3((unsigned)B), dim3(kGreedyConfTile), 0, st, row_max, row_arg, lens, T, blank, tokens,
                     n_tokens, tok_start, tok_end, tok_mean, tok_min, utt_sum, n_nonblank, conf);
  LASR_LAUNCH_CHECK("greedy_conf_collapse_kernel");
  return 0;
}
