// Voice-activity segmentation of long recordings on the device, and the gather from segments to batch rows (segment.h has the level
// function, the parameter conversion and the checks; DESIGN.md "Inference: long recordings" states the rule).  Everything after the
// PCM16 quantisation of a sample is integer arithmetic, so the result does not depend on the order of any sum.
//
// lasr_vad_segment is a memset and two launches:
//   vad_levels_kernel  grid (ceil(F / 64), B), 4 waves: a wave takes one frame at a time - 160 samples, q^2 summed per lane in 32 bits
//                      (three values of at most 2^30) and across the wave in 64 - and lane 0 stores the frame's level and counts it
//                      in the workgroup's 512-bin LDS histogram, flushed with integer atomics at the end.
//   vad_rows_kernel    one 1024-thread workgroup per row: thread 0 takes the noise floor from the 512 bins; then every pass is the
//                      same sweep (sweep_scan): kSweep items per iteration, four per thread, an exclusive prefix sum of a per-item
//                      value over the workgroup with the carry of the earlier sweeps, and a per-item emit that scatters by that prefix.
//                        A  frames -> runs of lev >= off: the prefix counts run starts (high word) and frames >= on (low word); a
//                           run's first frame writes its start, its last frame its end, both at (starts so far) - 1
//                        B  hysteresis: keep the runs whose on-count grew between start and end (compaction)
//                        C  close: run i heads a group unless it starts < min_silence after run i - 1 ends - a LOCAL condition, as
//                           the merged run ends where its last member ends; heads write starts, tails write ends at (heads so far) - 1
//                        D  open: keep groups of >= min_speech frames (compaction), padded on the way out
//                        E  pad merge: as C with the condition start <= previous end
//                        F  split: a wave per run walks the cut loop (the 64 lanes search a window for its first lowest frame:
//                           min over (level << 32 | frame)), once to count the pieces; a sweep turns counts into offsets; the same
//                           walk again writes the pieces.
//                      The run lists live in the workspace (two lists, ping-pong); F may be far larger than a sweep, or 0.
// lasr_segment_gather copies the segments of a HOST table: up to 256 table entries travel by value in a launch's arguments.
#include "common.h"
#include "segment.h"

using namespace lasr;

static_assert(sizeof(lasr_vad_params) == sizeof(segment::Params), "lasr_vad_params is segment::Params, field for field");
static_assert(LASR_VAD_LEVELS == segment::kLevels, "one bin count");

namespace {

constexpr int kHop = segment::kHop;
constexpr int kBins = segment::kLevels;
constexpr int kLevThreads = 256, kLevWaves = kLevThreads / 64, kLevFrames = 64;   // frames per workgroup of the wide pass
constexpr int kRowThreads = 1024, kRowWaves = kRowThreads / 64, kItems = 4;
constexpr int kSweep = kRowThreads * kItems;                                      // items one sweep of the row kernel takes
constexpr int kLists = 6;                                                         // int32 arrays of `cap` entries per row
constexpr int kGatherChunk = 256;                                                 // table entries per launch (3 KB of arguments)
constexpr int kGatherThreads = 256;

__device__ __forceinline__ int quantise(int16_t v) { return v; }
__device__ __forceinline__ int quantise(float x) {         // clamp(rint(x * 32768), -32768, 32767), half to even; a NaN gives -32768
  return (int)fminf(fmaxf(rintf(x * 32768.0f), -32768.0f), 32767.0f);
}

__device__ __forceinline__ int64_t row_len(const int32_t* __restrict__ lens, int64_t b, int64_t L) {
  const int64_t n = lens ? (int64_t)lens[b] : L;
  return n < 0 ? 0 : (n > L ? L : n);
}

template <typename T>
__global__ __launch_bounds__(kLevThreads) void vad_levels_kernel(const T* __restrict__ wave, int64_t pitch, const int32_t* __restrict__ lens,
                                                                 int64_t L, int64_t Fp, uint16_t* __restrict__ lev,
                                                                 uint16_t* __restrict__ levels_out, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kBins];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = blockIdx.y;
  for (int i = tid; i < kBins; i += kLevThreads) h[i] = 0;
  __syncthreads();
  const int64_t len = row_len(lens, b, L);
  const int64_t F = (len + kHop - 1) / kHop;
  const T* __restrict__ x = wave + b * pitch;
  for (int k = 0; k < kLevFrames / kLevWaves; ++k) {
    const int64_t f = (int64_t)blockIdx.x * kLevFrames + k * kLevWaves + w;        // uniform over the wave
    if (f >= Fp) break;
    if (f >= F) {                                          // past the row's end: only the diagnostic output is defined there
      if (lane == 0 && levels_out) levels_out[b * Fp + f] = 0;
      continue;
    }
    const int64_t s0 = f * kHop;
    uint32_t acc = 0;
#pragma unroll
    for (int r = 0; r < (kHop + 63) / 64; ++r) {
      const int i = lane + 64 * r;
      if (i < kHop && s0 + i < len) {
        const int q = quantise(x[s0 + i]);
        acc += (uint32_t)(q * q);
      }
    }
    unsigned long long e = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    if (lane == 0) {
      const int lv = segment::level(e);
      lev[b * Fp + f] = (uint16_t)lv;
      if (levels_out) levels_out[b * Fp + f] = (uint16_t)lv;
      atomicAdd(&h[lv], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < kBins; i += kLevThreads)
    if (h[i]) atomicAdd(&hist[b * kBins + i], h[i]);
}

struct RowShared {
  unsigned long long wave_tot[kRowWaves];
  uint32_t hist[kBins];
  int floor_lv;
};

// For i in [0, n): emit(i, sum of value(j) over j < i, value(i)), by the whole workgroup; returns the sum over [0, n).  value() may
// pack two counters into the halves of its 64 bits (neither overflows its half: n < 2^31).  Ends on a barrier: what emit wrote is
// visible to the workgroup afterwards.  n is uniform.
template <typename V, typename E>
__device__ __forceinline__ unsigned long long sweep_scan(int n, RowShared& sh, V value, E emit) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long carry = 0;
  for (int base = 0; base < n; base += kSweep) {
    const int i0 = base + tid * kItems;
    unsigned long long v[kItems], sum = 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      v[j] = i0 + j < n ? value(i0 + j) : 0ull;
      sum += v[j];
    }
    unsigned long long inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) sh.wave_tot[w] = inc;
    __syncthreads();
    unsigned long long pre = carry, tot = 0;
#pragma unroll
    for (int k = 0; k < kRowWaves; ++k) {
      const unsigned long long t = sh.wave_tot[k];
      if (k < w) pre += t;
      tot += t;
    }
    pre += inc - sum;
#pragma unroll
    for (int j = 0; j < kItems; ++j)
      if (i0 + j < n) {
        emit(i0 + j, pre, v[j]);
        pre += v[j];
      }
    carry += tot;
    __syncthreads();
  }
  return carry;
}

// The split loop of one run [s, e), by one wave; returns the number of pieces.  EMIT: piece k goes to row `o + k` of segs when that
// is below max_segments.
template <bool EMIT>
__device__ __forceinline__ int split_run(const uint16_t* __restrict__ lv, int s, int e, int max_frames, int lane, int64_t len,
                                         int32_t* __restrict__ segs, int64_t max_segments, int64_t o) {
  int cnt = 0;
  auto put = [&](int a, int z) {
    if (EMIT && lane == 0 && o + cnt < max_segments) {
      const int64_t end = (int64_t)z * kHop;
      segs[2 * (o + cnt)] = (int32_t)((int64_t)a * kHop);
      segs[2 * (o + cnt) + 1] = (int32_t)(end < len ? end : len);
    }
    ++cnt;
  };
  while (e - s > max_frames) {                             // the window [s + max_frames / 2, s + max_frames) lies inside the run
    unsigned long long key = ~0ull;
    for (int n = s + max_frames / 2 + lane; n < s + max_frames; n += 64) {
      const unsigned long long kn = ((unsigned long long)lv[n] << 32) | (uint32_t)n;
      key = kn < key ? kn : key;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long t = __shfl_xor(key, d, 64);
      key = t < key ? t : key;
    }
    const int c = (int)(uint32_t)key;                      // > s, as max_frames >= 2
    put(s, c);
    s = c;
  }
  put(s, e);
  return cnt;
}

__global__ __launch_bounds__(kRowThreads) void vad_rows_kernel(const int32_t* __restrict__ lens, int64_t L, int64_t Fp, int64_t cap,
                                                               lasr_vad_params p, const uint16_t* __restrict__ lev_all,
                                                               const uint32_t* __restrict__ hist_all, int32_t* __restrict__ lists,
                                                               int32_t* __restrict__ segs_all, int64_t max_segments,
                                                               int32_t* __restrict__ n_segs, int32_t* __restrict__ floor_out) {
  __shared__ RowShared sh;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = blockIdx.x;
  const int64_t len = row_len(lens, b, L);
  const int F = (int)((len + kHop - 1) / kHop);
  const uint16_t* __restrict__ lv = lev_all + b * Fp;
  int32_t* xs = lists + b * kLists * cap;                  // list X: start, end, on-count at start, on-count at end
  int32_t *xe = xs + cap, *xa = xe + cap, *xb = xa + cap;
  int32_t *ys = xb + cap, *ye = ys + cap;                  // list Y: start, end
  int32_t* __restrict__ segs = segs_all + b * max_segments * 2;

  // noise floor: the rank-th smallest level of the row
  for (int i = tid; i < kBins; i += kRowThreads) sh.hist[i] = F > 0 ? hist_all[b * kBins + i] : 0u;
  __syncthreads();
  if (tid == 0) {
    int64_t rank = ((int64_t)F * p.floor_permille + 999) / 1000;
    if (rank < 1) rank = 1;
    int64_t cum = 0;
    int fl = 0;
    for (int l = 0; l < kBins; ++l) {
      cum += sh.hist[l];
      if (cum >= rank) { fl = l; break; }
    }
    sh.floor_lv = fl;
    if (floor_out) floor_out[b] = fl;
  }
  __syncthreads();
  const int fl = sh.floor_lv;
  const int base = fl < p.min_level ? p.min_level : (fl > p.max_floor_level ? p.max_floor_level : fl);
  const int on = base + p.on_steps, off = base + p.off_steps;

  // A: maximal runs of lev >= off, with the count of frames >= on before their start and up to their end
  const int R0 = (int)(sweep_scan(F, sh,
      [&](int n) -> unsigned long long {
        const int l = lv[n];
        const bool start = l >= off && !(n > 0 && lv[n - 1] >= off);
        return ((unsigned long long)start << 32) | (unsigned long long)(l >= on);
      },
      [&](int n, unsigned long long pre, unsigned long long v) {
        if (lv[n] < off) return;
        const int k = (int)(pre >> 32) + (int)(v >> 32) - 1;          // the run this frame lies in
        const int32_t seen = (int32_t)(uint32_t)pre;
        if (v >> 32) { xs[k] = n; xa[k] = seen; }
        if (n + 1 == F || lv[n + 1] < off) { xe[k] = n + 1; xb[k] = seen + (int32_t)(v & 1); }
      }) >> 32);
  // B: hysteresis
  const int R1 = (int)sweep_scan(R0, sh, [&](int i) -> unsigned long long { return xb[i] > xa[i]; },
      [&](int i, unsigned long long pre, unsigned long long v) {
        if (v) { ys[pre] = xs[i]; ye[pre] = xe[i]; }
      });
  // C: close gaps shorter than min_silence
  {
    auto head = [&](int i) { return i == 0 || ys[i] - ye[i - 1] >= p.min_silence; };
    const int R2 = (int)sweep_scan(R1, sh, [&](int i) -> unsigned long long { return head(i); },
        [&](int i, unsigned long long pre, unsigned long long v) {
          const int g = (int)pre + (int)v - 1;
          if (v) xs[g] = ys[i];
          if (i + 1 == R1 || head(i + 1)) xe[g] = ye[i];
        });
    // D: drop runs shorter than min_speech, pad the rest
    const int R3 = (int)sweep_scan(R2, sh, [&](int i) -> unsigned long long { return xe[i] - xs[i] >= p.min_speech; },
        [&](int i, unsigned long long pre, unsigned long long v) {
          if (!v) return;
          const int s = xs[i] - p.pad, e = xe[i] + p.pad;
          ys[pre] = s < 0 ? 0 : s;
          ye[pre] = e > F ? F : e;
        });
    // E: padded runs that overlap or touch are one run
    auto phead = [&](int i) { return i == 0 || ys[i] > ye[i - 1]; };
    const int R4 = (int)sweep_scan(R3, sh, [&](int i) -> unsigned long long { return phead(i); },
        [&](int i, unsigned long long pre, unsigned long long v) {
          const int g = (int)pre + (int)v - 1;
          if (v) xs[g] = ys[i];
          if (i + 1 == R3 || phead(i + 1)) xe[g] = ye[i];
        });
    // F: split runs longer than max_frames; ys = pieces per run, then the offset of its first piece
    for (int i = w; i < R4; i += kRowWaves) {
      const int c = split_run<false>(lv, xs[i], xe[i], p.max_frames, lane, len, segs, max_segments, 0);
      if (lane == 0) ys[i] = c;
    }
    __syncthreads();
    const unsigned long long total = sweep_scan(R4, sh, [&](int i) -> unsigned long long { return (unsigned long long)ys[i]; },
        [&](int i, unsigned long long pre, unsigned long long) { ys[i] = (int32_t)pre; });
    for (int i = w; i < R4; i += kRowWaves) split_run<true>(lv, xs[i], xe[i], p.max_frames, lane, len, segs, max_segments, ys[i]);
    if (tid == 0) n_segs[b] = (int32_t)total;
  }
}

struct GatherChunk {
  int32_t e[kGatherChunk][3];
};

template <typename T>
__global__ __launch_bounds__(kGatherThreads) void segment_gather_kernel(const T* __restrict__ wave, int64_t pitch, GatherChunk tab,
                                                                        T* __restrict__ out, int64_t out_pitch,
                                                                        int32_t* __restrict__ out_lens) {
  const int i = blockIdx.y;
  const int64_t row = tab.e[i][0], start = tab.e[i][1], n = (int64_t)tab.e[i][2] - start;
  const T* __restrict__ x = wave + row * pitch + start;
  T* __restrict__ y = out + (int64_t)i * out_pitch;
  if (blockIdx.x == 0 && threadIdx.x == 0) out_lens[i] = (int32_t)n;
  for (int64_t j = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x; j < out_pitch; j += (int64_t)gridDim.x * kGatherThreads)
    y[j] = j < n ? x[j] : (T)0;
}

struct VadLayout {
  int64_t Fp, cap;
  size_t hist_off, lists_off, lev_off, bytes;
};

VadLayout vad_layout(int64_t B, int64_t L) {
  VadLayout v;
  v.Fp = segment::num_frames(L);
  v.cap = v.Fp / 2 + 1;                                    // runs are separated by at least one frame
  v.hist_off = 0;
  v.lists_off = align_up((size_t)B * kBins * 4, 16);
  v.lev_off = v.lists_off + align_up((size_t)B * kLists * (size_t)v.cap * 4, 16);
  v.bytes = v.lev_off + align_up((size_t)B * (size_t)v.Fp * 2, 16);
  return v;
}

bool vad_shape_ok(int64_t B, int64_t L) { return B >= 0 && B <= 65535 && L >= 0 && L <= segment::kMaxLen; }

}  // namespace

extern "C" int lasr_vad_params_from(double on_db, double off_db, int floor_permille, double min_level_db, double max_floor_db,
                                    double min_silence_s, double min_speech_s, double pad_s, double max_segment_s, lasr_vad_params* out) {
  LASR_CHECK_ARG(out, "lasr_vad_params_from: null pointer");
  std::string err;
  segment::Params p;
  if (segment::from(on_db, off_db, floor_permille, min_level_db, max_floor_db, min_silence_s, min_speech_s, pad_s, max_segment_s, &p, &err) !=
      segment::kOk)
    return fail(LASR_E_ARG, "lasr_vad_params_from: %s", err.c_str());
  memcpy(out, &p, sizeof(p));
  return 0;
}

extern "C" int64_t lasr_vad_sweep(void) { return kSweep; }

extern "C" size_t lasr_vad_workspace_bytes(int64_t B, int64_t L) {
  if (!vad_shape_ok(B, L)) {
    fail(LASR_E_SHAPE, "lasr_vad_workspace_bytes: at most 65535 rows of fewer than 2^31 samples");
    return 0;
  }
  return vad_layout(B, L).bytes;
}

extern "C" int lasr_vad_segment(const void* wave, int wave_dtype, int64_t pitch, const int32_t* sample_lens, int64_t B, int64_t L,
                                const lasr_vad_params* params, int32_t* segs, int64_t max_segments, int32_t* n_segs, int32_t* floor_out,
                                uint16_t* levels_out, void* workspace, size_t workspace_bytes, void* stream) {
  LASR_CHECK_ARG(params && n_segs && (wave || L == 0 || B == 0), "lasr_vad_segment: null pointer");
  LASR_CHECK_ARG(wave_dtype == LASR_WAVE_F32 || wave_dtype == LASR_WAVE_PCM16, "lasr_vad_segment: wave_dtype is LASR_WAVE_F32 or LASR_WAVE_PCM16");
  LASR_CHECK_ARG(B >= 0 && L >= 0 && pitch >= 0 && (pitch == 0 || pitch >= L), "lasr_vad_segment: negative size or 0 < pitch < L");
  LASR_CHECK_ARG(max_segments >= 0 && (segs || max_segments == 0), "lasr_vad_segment: max_segments < 0 or no segs to hold them");
  LASR_CHECK_SHAPE(vad_shape_ok(B, L) && max_segments < ((int64_t)1 << 31), "lasr_vad_segment: at most 65535 rows of fewer than 2^31 samples");
  std::string err;
  segment::Params p;
  memcpy(&p, params, sizeof(p));
  if (segment::check(p, &err) != segment::kOk) return fail(LASR_E_ARG, "lasr_vad_segment: %s", err.c_str());
  if (B == 0) return 0;
  const VadLayout v = vad_layout(B, L);
  LASR_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0, "lasr_vad_segment: the workspace must be 16-byte aligned");
  if (workspace_bytes < v.bytes) return fail(LASR_E_WORKSPACE, "lasr_vad_segment: workspace of %zu bytes, need %zu", workspace_bytes, v.bytes);
  char* ws = static_cast<char*>(workspace);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + v.hist_off);
  int32_t* lists = reinterpret_cast<int32_t*>(ws + v.lists_off);
  uint16_t* lev = reinterpret_cast<uint16_t*>(ws + v.lev_off);
  hipStream_t st = as_stream(stream);
  const int64_t row_pitch = pitch ? pitch : L;
  if (v.Fp > 0) {
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * kBins * 4, st);
    if (e != hipSuccess) return hip_fail(e, "lasr_vad_segment (memset)");
    const dim3 grid((unsigned)cdiv(v.Fp, kLevFrames), (unsigned)B);
    if (wave_dtype == LASR_WAVE_F32)
      hipLaunchKernelGGL(vad_levels_kernel<float>, grid, dim3(kLevThreads), 0, st, static_cast<const float*>(wave), row_pitch, sample_lens, L,
                         v.Fp, lev, levels_out, hist);
    else
      hipLaunchKernelGGL(vad_levels_kernel<int16_t>, grid, dim3(kLevThreads), 0, st, static_cast<const int16_t*>(wave), row_pitch, sample_lens,
                         L, v.Fp, lev, levels_out, hist);
    LASR_LAUNCH_CHECK("lasr_vad_segment (levels)");
  }
  hipLaunchKernelGGL(vad_rows_kernel, dim3((unsigned)B), dim3(kRowThreads), 0, st, sample_lens, L, v.Fp, v.cap, *params, lev, hist, lists, segs,
                     max_segments, n_segs, floor_out);
  LASR_LAUNCH_CHECK("lasr_vad_segment (rows)");
  return 0;
}

extern "C" int lasr_segment_gather(const void* wave, int wave_dtype, int64_t pitch, const int32_t* table, int64_t n, void* out,
                                   int64_t out_pitch, int32_t* out_lens, void* stream) {
  LASR_CHECK_ARG(n >= 0 && pitch >= 0 && out_pitch >= 0, "lasr_segment_gather: negative size");
  LASR_CHECK_ARG(wave_dtype == LASR_WAVE_F32 || wave_dtype == LASR_WAVE_PCM16, "lasr_segment_gather: wave_dtype is LASR_WAVE_F32 or LASR_WAVE_PCM16");
  if (n == 0) return 0;
  LASR_CHECK_ARG(wave && table && out_lens && (out || out_pitch == 0), "lasr_segment_gather: null pointer");
  LASR_CHECK_SHAPE(out_pitch < ((int64_t)1 << 31), "lasr_segment_gather: rows of fewer than 2^31 samples");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t row = table[3 * i], s = table[3 * i + 1], e = table[3 * i + 2];
    LASR_CHECK_ARG(row >= 0 && s >= 0 && e >= s, "lasr_segment_gather: table[%lld] = (%lld, %lld, %lld) is no segment", (long long)i,
                   (long long)row, (long long)s, (long long)e);
    LASR_CHECK_SHAPE(e - s <= out_pitch, "lasr_segment_gather: segment %lld holds %lld samples, out_pitch is %lld", (long long)i,
                     (long long)(e - s), (long long)out_pitch);
  }
  hipStream_t st = as_stream(stream);
  const int64_t tiles = cdiv(out_pitch > 0 ? out_pitch : 1, kGatherThreads * 4);
  for (int64_t i0 = 0; i0 < n; i0 += kGatherChunk) {
    const int m = (int)(n - i0 < kGatherChunk ? n - i0 : kGatherChunk);
    GatherChunk tab;
    memset(&tab, 0, sizeof(tab));
    memcpy(tab.e, table + 3 * i0, (size_t)m * 12);
    const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024), (unsigned)m);
    if (wave_dtype == LASR_WAVE_F32)
      hipLaunchKernelGGL(segment_gather_kernel<float>, grid, dim3(kGatherThreads), 0, st, static_cast<const float*>(wave), pitch, tab,
                         static_cast<float*>(out) + i0 * out_pitch, out_pitch, out_lens + i0);
    else
      hipLaunchKernelGGL(segment_gather_kernel<int16_t>, grid, dim3(kGatherThreads), 0, st, static_cast<const int16_t*>(wave), pitch, tab,
                         static_cast<int16_t*>(out) + i0 * out_pitch, out_pitch, out_lens + i0);
    LASR_LAUNCH_CHECK("lasr_segment_gather");
  }
  return 0;
}
