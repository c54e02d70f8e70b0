// Waveform augmentation on the device: reverberation with a room impulse response (a long FIR) and additive noise at a drawn SNR,
// over a batch of rows, each row with its own parameter word (rir_id, noise_id, noise_start, snr_cdb).  wave_aug.h builds the RIR
// bank image on the host; DESIGN.md "Noise and reverberation" has the definition.
//   y[j] = sum_{k < K} h[k] * x[j + d - k]   (x = 0 outside [0, n));   v[j] = noise[off + (s + j) mod len]
//   out[j] = g_s * y[j] + g_n * v[j],  g_s = sqrt(E_x / E_y),  g_n = sqrt(E_x / (E_n * 10^(snr / 10)))
// Three launches on the caller's stream, nothing allocated, nothing synchronised:
//   1. energy_fir_kernel, grid (tiles, B): the tile's partial E_x and E_n, and - on rows with an RIR - the FIR of the tile into the
//      workspace (f32) with its partial E_y.  A thread keeps 4 CONSECUTIVE outputs in each half of the tile and a sliding window
//      of staged samples in registers.  The LDS holds the two halves interleaved - (x[i], x[i + kTile / 2]) as one 8-byte pair -
//      so that one packed fma serves the same output of both halves and a window shift moves whole register pairs; the pairs of
//      a block of 4 are split over two planes so that a lane's 16-byte reads are 16 bytes apart from its neighbour's (no bank
//      conflict).  Per 4 taps a thread reads two 16-byte LDS words and issues 16 packed fmas (32 fmas); the taps are
//      workgroup-uniform, read through the scalar path.  Taps are walked in chunks of kChunk so that the staged span fits in LDS;
//      a chunk whose whole span lies outside the row is skipped.  f32 accumulation, ascending k, one fma per tap.
//   2. gains_kernel, grid B: sums the row's partials in tile order (f64, no atomics), writes stats, out_lens and the row's plan
//      (what to do, gains rounded once to f32) into the workspace.
//   3. mix_kernel, grid (tiles, B): out = g_s * y + g_n * v, zeros past n; identity rows are copied; bad rows are zeros.  It reads
//      the plan and, on reverberated rows, only the workspace's y - so `out` may be `in`.
#include "common.h"
#include "wave_aug.h"
#include "wave_sample.h"

using namespace lasr;

namespace {

constexpr int kThreads = 256;
constexpr int kR = wave_aug::kOutPerThread;
constexpr int kTile = wave_aug::kTile;
constexpr int kChunk = wave_aug::kChunk;
constexpr int kHalf = kTile / 2;
constexpr int kBlocks = (kHalf + kChunk) / 4;          // staged blocks of 4 pairs per plane
static_assert(kR == 8 && kTile == kThreads * kR && wave_aug::kTapPad == 8, "the FIR keeps 2 x 4 accumulators per thread and walks 8 taps per step");

typedef float v2f __attribute__((ext_vector_type(2)));

enum { kRowBad = 0, kRowCopy = 1, kRowMix = 2 };

struct Args {
  const int32_t* bank; int64_t bank_words;
  const void* noise; int noise_dtype; const int32_t* clips; int n_clips; int64_t noise_total;
  const int32_t* in_lens; const int32_t* params; int64_t in_pitch, L;
};

// what a row asks for, decoded the same way by every workgroup that touches it; every field is uniform over the workgroup
struct Row {
  int status;            // kRowBad: zeros, length 0; kRowCopy: neither id set; kRowMix
  int n;                 // valid samples (kRowCopy: the lead-in sample included)
  int word;              // the length word as given
  int K, d, tap_off;     // K = 0: no reverb
  int noise_off, noise_len, noise_start;      // noise_len = 0: no noise
  int snr_cdb;
};

__device__ __forceinline__ Row decode(const Args& a, int64_t b) {
  Row r = {};
  const int32_t* p = a.params + 4 * b;
  const int rir = p[0], nid = p[1], start = p[2];
  r.snr_cdb = p[3];
  r.word = a.in_lens[b];
  const int n_word = r.word < 0 ? 0 : (r.word & (LASR_LEN_LEAD - 1));
  if (rir < 0 && nid < 0) {                        // identity: a copy, the lead-in sample and its flag included
    const int lead = (r.word > 0 && (r.word & LASR_LEN_LEAD)) ? 1 : 0;
    int64_t n = (int64_t)n_word + lead;
    if (n > a.L) { n = a.L; r.word = (int)n; }      // (cut at L: the flag goes with the cut)
    r.n = (int)n;
    r.status = kRowCopy;
    return r;
  }
  r.n = (int64_t)n_word < a.L ? n_word : (int)a.L;
  bool ok = true;
  if (rir >= 0) {
    const int32_t* bk = a.bank;
    ok = bk != nullptr && a.bank_words >= wave_aug::kHeaderWords && (uint32_t)bk[0] == wave_aug::kMagic && bk[1] >= 0 &&
         bk[1] <= wave_aug::kMaxRir && rir < bk[1] && (int64_t)bk[2] <= a.bank_words;
    if (ok) {
      const int32_t* e = bk + 4 + 4 * rir;
      r.K = e[0]; r.d = e[1]; r.tap_off = e[2];
      ok = wave_aug::entry_ok(r.K, r.d, r.tap_off, bk[2]);
    }
  }
  if (ok && nid >= 0) {
    ok = a.noise != nullptr && a.clips != nullptr && nid < a.n_clips;
    if (ok) {
      r.noise_off = a.clips[2 * nid]; r.noise_len = a.clips[2 * nid + 1]; r.noise_start = start;
      ok = r.noise_off >= 0 && r.noise_len >= 1 && (int64_t)r.noise_off + r.noise_len <= a.noise_total && start >= 0 && start < r.noise_len;
    }
  }
  if (!ok) { r = Row(); r.status = kRowBad; return r; }
  r.status = kRowMix;
  return r;
}

__device__ __forceinline__ float noise_at(const Args& a, int64_t i) {
  return a.noise_dtype == LASR_WAVE_F32 ? static_cast<const float*>(a.noise)[i]
                                        : (float)static_cast<const int16_t*>(a.noise)[i] * (1.0f / 32768.0f);
}

// sum over the workgroup in a fixed order (a tree over thread ids): the same bits on every run
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// a block of 4 staged pairs: a = pairs 0, 1 (plane A), b = pairs 2, 3 (plane B); a pair = (sample of half 0, sample of half 1)
struct Blk { float4 a, b; };

// 4 taps h[0..3] against the window v = (lo, hi), lo lowest: tap u meets pair v[3 - u + r] for output r of both halves
__device__ __forceinline__ void fir4(v2f (&acc)[4], const Blk& lo, const Blk& hi, const float4& h) {
  const v2f v[7] = {{lo.a.x, lo.a.y}, {lo.a.z, lo.a.w}, {lo.b.x, lo.b.y}, {lo.b.z, lo.b.w}, {hi.a.x, hi.a.y}, {hi.a.z, hi.a.w}, {hi.b.x, hi.b.y}};
  const float t[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = __builtin_elementwise_fma((v2f){t[u], t[u]}, v[3 - u + r], acc[r]);
}

template <typename TI>
__global__ __launch_bounds__(kThreads) void energy_fir_kernel(Args a, const TI* __restrict__ in, float* __restrict__ ybuf, int64_t y_pitch,
                                                              double* __restrict__ partial, int n_tiles) {
  __shared__ float4 xa[kBlocks], xb[kBlocks];          // pair i of the span: plane (i & 2), block i >> 2, slot i & 1
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int tile = blockIdx.x;
  const Row row = decode(a, b);
  double* part = partial + (b * n_tiles + tile) * 3;
  const int64_t j0 = (int64_t)tile * kTile;
  if (row.status == kRowBad || j0 >= row.n) {      // uniform
    if (tid < 3) part[tid] = 0.0;
    return;
  }
  const TI* __restrict__ x = in + b * a.in_pitch;
  const int n = row.n;

  // E_x and E_n of the tile
  double ex = 0.0, en = 0.0;
  int64_t pos = 0;
  int step = 0;
  if (row.noise_len) {
    pos = ((int64_t)row.noise_start + j0 + tid) % row.noise_len;
    step = kThreads % row.noise_len;
  }
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int64_t j = j0 + tid + r * kThreads;
    if (j < n) {
      const double xv = (double)load_sample(x + j);
      ex += xv * xv;
      if (row.noise_len) {
        const double nv = (double)noise_at(a, row.noise_off + pos);
        en += nv * nv;
      }
    }
    pos += step;
    if (pos >= row.noise_len) pos -= row.noise_len;
  }
  ex = block_sum(ex, red);
  if (row.noise_len) en = block_sum(en, red);
  if (row.status == kRowCopy || row.K == 0) {
    if (tid == 0) { part[0] = ex; part[1] = ex; part[2] = en; }
    return;
  }

  // the FIR: thread tid owns outputs j0 + 4 tid + r and j0 + kHalf + 4 tid + r, r < 4
  const float* __restrict__ h = reinterpret_cast<const float*>(a.bank) + row.tap_off;
  v2f acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = (v2f){0.0f, 0.0f};
  const int K = row.K;
  for (int k0 = 0; k0 < K; k0 += kChunk) {
    const int kn = K - k0 < kChunk ? K - k0 : kChunk;
    const int kp = (kn + wave_aug::kTapPad - 1) / wave_aug::kTapPad * wave_aug::kTapPad;     // taps past K are stored as zeros
    const int64_t in0 = j0 + row.d - k0 - (kp - 1);       // input index of pair 0's first sample
    const int pairs = kHalf + kp;                         // <= 4 kBlocks
    if (in0 >= n || in0 + kHalf + pairs <= 0) continue;   // nothing but zeros under this chunk
    __syncthreads();                                      // the previous chunk has been read
    for (int i = tid; i < pairs; i += kThreads) {
      const int64_t i0 = in0 + i, i1 = i0 + kHalf;
      const float v0 = (i0 >= 0 && i0 < n) ? load_sample(x + i0) : 0.0f;
      const float v1 = (i1 >= 0 && i1 < n) ? load_sample(x + i1) : 0.0f;
      float* plane = reinterpret_cast<float*>((i & 2) ? xb : xa);
      *reinterpret_cast<float2*>(plane + (i >> 2) * 4 + (i & 1) * 2) = make_float2(v0, v1);
    }
    __syncthreads();
    const float4* __restrict__ h4 = reinterpret_cast<const float4*>(h + k0);
    const float4* pa = xa + tid + kp / 4 - 1;             // tap 0's lowest block
    const float4* pb = xb + tid + kp / 4 - 1;
    Blk x0, x1 = {pa[1], pb[1]};
    for (int g = 0; g < kp / 4; g += 2) {
      x0 = {pa[0], pb[0]};   fir4(acc, x0, x1, h4[g]);
      x1 = {pa[-1], pb[-1]}; fir4(acc, x1, x0, h4[g + 1]);
      pa -= 2; pb -= 2;
    }
  }
  float* __restrict__ y = ybuf + b * y_pitch + j0 + tid * 4;        // y_pitch is a multiple of kTile: whole tiles are stored
  *reinterpret_cast<float4*>(y) = make_float4(acc[0].x, acc[1].x, acc[2].x, acc[3].x);
  *reinterpret_cast<float4*>(y + kHalf) = make_float4(acc[0].y, acc[1].y, acc[2].y, acc[3].y);
  double ey = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (j0 + tid * 4 + r < n) ey += (double)acc[r].x * (double)acc[r].x;
    if (j0 + kHalf + tid * 4 + r < n) ey += (double)acc[r].y * (double)acc[r].y;
  }
  ey = block_sum(ey, red);
  if (tid == 0) { part[0] = ex; part[1] = ey; part[2] = en; }
}

// plan of a row in the workspace: 8 words {status, n, g_s, g_n, noise_off, noise_len, noise_start, reverb}
__global__ __launch_bounds__(64) void gains_kernel(Args a, const double* __restrict__ partial, int n_tiles, int32_t* __restrict__ plan,
                                                   int32_t* __restrict__ out_lens, double* __restrict__ stats) {
  __shared__ double e[3];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const Row row = decode(a, b);
  if (tid < 3) {
    double s = 0.0;
    const double* p = partial + b * n_tiles * 3 + tid;
    for (int t = 0; t < n_tiles; ++t) s += p[3 * t];
    e[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  const double ex = e[0], ey = e[1], en = e[2];
  float gs = 0.0f, gn = 0.0f;
  if (row.status == kRowMix) {
    gs = row.K ? (ey > 0.0 ? (float)sqrt(ex / ey) : 0.0f) : 1.0f;
    if (row.noise_len && ex > 0.0 && en > 0.0) gn = (float)sqrt(ex / (en * pow(10.0, (double)row.snr_cdb / 1000.0)));
  }
  int32_t* pl = plan + 8 * b;
  pl[0] = row.status; pl[1] = row.n; pl[2] = __float_as_int(gs); pl[3] = __float_as_int(gn);
  pl[4] = row.noise_off; pl[5] = row.noise_len; pl[6] = row.noise_start; pl[7] = row.K;
  stats[3 * b] = ex; stats[3 * b + 1] = ey; stats[3 * b + 2] = en;
  out_lens[b] = row.status == kRowCopy ? row.word : row.n;        // kRowBad: n = 0
}

template <typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void mix_kernel(Args a, const TI* in, const float* __restrict__ ybuf, int64_t y_pitch,
                                                       const int32_t* __restrict__ plan, TO* out, int64_t out_pitch) {
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int32_t* pl = plan + 8 * b;
  const int status = pl[0], n = pl[1], noise_off = pl[4], noise_len = pl[5], noise_start = pl[6], reverb = pl[7];
  const float gs = __int_as_float(pl[2]), gn = __int_as_float(pl[3]);
  const TI* x = in + b * a.in_pitch;                // (no __restrict__: out may be in)
  TO* o = out + b * out_pitch;
  const float* __restrict__ y = ybuf + b * y_pitch;
  const int64_t j0 = (int64_t)blockIdx.x * kTile;
  int64_t pos = 0;
  int step = 0;
  if (noise_len) {
    pos = ((int64_t)noise_start + j0 + tid) % noise_len;
    step = kThreads % noise_len;
  }
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int64_t j = j0 + tid + r * kThreads;
    if (j < n) {
      if (status == kRowCopy) copy_sample(o + j, x + j);
      else {
        const float s = gs * (reverb ? y[j] : load_sample(x + j));
        store_sample(o + j, noise_len ? fmaf(gn, noise_at(a, noise_off + pos), s) : s);
      }
    } else if (j < a.L) store_sample(o + j, 0.0f);
    pos += step;
    if (pos >= noise_len) pos -= noise_len;
  }
}

int host_rc(int rc, const std::string& err) { return rc == wave_aug::kOk ? 0 : fail(LASR_E_ARG, "%s", err.c_str()); }

int64_t tiles_of(int64_t L) { return L < 1 ? 1 : (L + kTile - 1) / kTile; }
// workspace: y (B rows of whole tiles, f32) | partials (B, tiles, 3) f64 | plans (B, 8) int32
size_t ws_y_bytes(int64_t B, int64_t L) { return (size_t)B * (size_t)tiles_of(L) * kTile * 4; }
size_t ws_partial_bytes(int64_t B, int64_t L) { return (size_t)B * (size_t)tiles_of(L) * 3 * 8; }

}  // namespace

extern "C" size_t lasr_rir_bank_bytes(const float* rirs, const int64_t* lens, int n_rir) {
  std::string err;
  const size_t n = wave_aug::bank_bytes(rirs, lens, n_rir, &err);
  if (!n) fail(LASR_E_ARG, "lasr_rir_bank_bytes: %s", err.c_str());
  return n;
}

extern "C" int lasr_rir_bank_write(const float* rirs, const int64_t* lens, int n_rir, void* host_dst, size_t bytes) {
  std::string err;
  return host_rc(wave_aug::bank_write(rirs, lens, n_rir, host_dst, bytes, &err), err);
}

extern "C" int64_t lasr_wave_augment_tile(void) { return kTile; }
extern "C" int64_t lasr_wave_augment_chunk(void) { return kChunk; }

extern "C" size_t lasr_wave_augment_workspace_bytes(int64_t B, int64_t L) {
  if (B < 0 || L < 0 || B > 65535 || L >= ((int64_t)1 << 31)) {
    fail(LASR_E_SHAPE, "lasr_wave_augment_workspace_bytes: at most 65535 rows of fewer than 2^31 samples");
    return 0;
  }
  return ws_y_bytes(B, L) + ws_partial_bytes(B, L) + (size_t)B * 32 + 64;
}

extern "C" int lasr_wave_augment(const void* rir_bank_dev, int64_t rir_bank_words, const void* noise_dev, int noise_dtype,
                                 const int32_t* noise_clips, int n_clips, int64_t noise_total, const void* in, int in_dtype,
                                 int64_t in_pitch, const int32_t* in_lens, const int32_t* params, void* out, int out_dtype,
                                 int64_t out_pitch, int64_t L, int32_t* out_lens, double* stats, int64_t B, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  auto wave = [](int dt) { return dt == LASR_WAVE_F32 || dt == LASR_WAVE_PCM16; };
  LASR_CHECK_ARG(in && in_lens && params && out && out_lens && stats && workspace, "lasr_wave_augment: null pointer");
  LASR_CHECK_ARG(wave(in_dtype) && wave(out_dtype) && wave(noise_dtype), "lasr_wave_augment: dtypes are LASR_WAVE_F32 or LASR_WAVE_PCM16");
  LASR_CHECK_ARG(B >= 0 && L >= 0 && in_pitch >= L && out_pitch >= L, "lasr_wave_augment: negative size or a pitch below L");
  LASR_CHECK_ARG(rir_bank_words >= 0 && rir_bank_words <= wave_aug::kMaxImageWords && n_clips >= 0 && noise_total >= 0 &&
                 noise_total < ((int64_t)1 << 31), "lasr_wave_augment: bank sizes out of range");
  LASR_CHECK_ARG(in != out || (in_dtype == out_dtype && in_pitch == out_pitch), "lasr_wave_augment: out may alias in only exactly");
  LASR_CHECK_SHAPE(B <= 65535 && L < ((int64_t)1 << 31) && in_pitch < ((int64_t)1 << 31), "lasr_wave_augment: at most 65535 rows of fewer than 2^31 samples");
  if (B == 0) return 0;
  LASR_CHECK_ARG(workspace_bytes >= lasr_wave_augment_workspace_bytes(B, L) && ((uintptr_t)workspace & 15) == 0,
                 "lasr_wave_augment: the workspace is smaller than lasr_wave_augment_workspace_bytes(B, L) or not 16-byte aligned");
  const int64_t tiles = tiles_of(L);
  char* ws = static_cast<char*>(workspace);
  float* ybuf = reinterpret_cast<float*>(ws);
  double* partial = reinterpret_cast<double*>(ws + ws_y_bytes(B, L));
  int32_t* plan = reinterpret_cast<int32_t*>(ws + ws_y_bytes(B, L) + ws_partial_bytes(B, L));
  const int64_t y_pitch = tiles * kTile;
  Args a = {static_cast<const int32_t*>(rir_bank_dev), rir_bank_dev ? rir_bank_words : 0, noise_dev, noise_dtype, noise_clips,
            noise_dev && noise_clips ? n_clips : 0, noise_total, in_lens, params, in_pitch, L};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles, (unsigned)B);
  if (in_dtype == LASR_WAVE_F32)
    hipLaunchKernelGGL((energy_fir_kernel<float>), grid, dim3(kThreads), 0, st, a, static_cast<const float*>(in), ybuf, y_pitch, partial, (int)tiles);
  else
    hipLaunchKernelGGL((energy_fir_kernel<int16_t>), grid, dim3(kThreads), 0, st, a, static_cast<const int16_t*>(in), ybuf, y_pitch, partial, (int)tiles);
  LASR_LAUNCH_CHECK("lasr_wave_augment (energies, FIR)");
  hipLaunchKernelGGL(gains_kernel, dim3((unsigned)B), dim3(64), 0, st, a, partial, (int)tiles, plan, out_lens, stats);
  LASR_LAUNCH_CHECK("lasr_wave_augment (gains)");
#define LASR_MIX(TI, TO)                                                                                                              \
  hipLaunchKernelGGL((mix_kernel<TI, TO>), grid, dim3(kThreads), 0, st, a, static_cast<const TI*>(in), ybuf, y_pitch, plan, \
                     static_cast<TO*>(out), out_pitch)
  if (in_dtype == LASR_WAVE_F32 && out_dtype == LASR_WAVE_F32) LASR_MIX(float, float);
  else if (in_dtype == LASR_WAVE_F32) LASR_MIX(float, int16_t);
  else if (out_dtype == LASR_WAVE_F32) LASR_MIX(int16_t, float);
  else LASR_MIX(int16_t, int16_t);
#undef LASR_MIX
  LASR_LAUNCH_CHECK("lasr_wave_augment (mix)");
  return 0;
}
