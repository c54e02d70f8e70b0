// Sample-rate conversion on the device: a polyphase windowed-sinc resampler over a batch of rows, each row with its own
// conversion out of a small bank (resample.h builds the bank image on the host; DESIGN.md "Resampling" has the definition).
//   out[j] = sum_k h[j % up][k] * x[(j / up) * down + k - width],  x = 0 outside [0, n_in),  n_out = ceil(n_in * up / down)
// One 256-thread workgroup produces a tile of nblk * up consecutive outputs of one row, i.e. nblk whole input blocks of `down`
// samples: the tile's input span is staged in LDS (f32; PCM16 is scaled by 1/32768 on the way in), the taps are read from the bank in
// its [tap][phase] layout - consecutive outputs of one input block differ only in the phase, so they read consecutive bank words
// and the SAME LDS word (a broadcast).  A conversion with many taps walks them in chunks of kc so that the staged span always fits;
// nblk and kc come from the bank header.  f32 accumulation, taps in ascending order, one fma per tap.
// The grid is sized from L_out alone (the bank lives on the device and is never read by the host): workgroup x of row b takes
// tiles x, x + gridDim.x, ... of that row's conversion.  No allocation, no host synchronisation.
#include "common.h"
#include "resample.h"
#include "wave_sample.h"

static_assert(lasr::resample::kMaxTile == 1024, "the kernel keeps 4 accumulators per thread of a 256-thread workgroup");

using namespace lasr;

namespace {

constexpr int kThreads = 256;
constexpr int kAcc = resample::kMaxTile / kThreads;

template <typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void resample_kernel(const int32_t* __restrict__ bank, const TI* __restrict__ in, int64_t in_pitch,
                                                            const int32_t* __restrict__ in_lens, const int32_t* __restrict__ conv_id,
                                                            TO* __restrict__ out, int64_t out_pitch, int64_t L_out,
                                                            int32_t* __restrict__ out_lens) {
  __shared__ float xs[resample::kSpanCap];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int cid = conv_id ? conv_id[b] : 0;
  const int n_conv = bank[1];
  bool ok = (uint32_t)bank[0] == resample::kMagic && n_conv >= 1 && n_conv <= resample::kMaxConv && cid >= 0 && cid < n_conv;
  const int32_t* e = bank + 16 + 8 * (ok ? cid : 0);      // read only when the header is one of ours
  if (ok) {     // ... and run only with a tiling that stays inside xs and ends: a damaged entry gives a row of zeros, like a bad id
    const int64_t u = e[0], d = e[1], w = e[2], t = e[3], o = e[4], nb = e[5], c = e[6];
    const bool ident = u == 1 && d == 1;
    ok = u >= 1 && u <= resample::kMaxFactor && d >= 1 && d <= resample::kMaxFactor && nb >= 1 && nb * u <= resample::kMaxTile &&
         (ident || (w >= 0 && t >= 1 && t * u <= resample::kMaxBankWords && o >= resample::kHeaderWords && c >= 1 && c <= resample::kMaxChunk &&
                    (nb - 1) * d + c <= resample::kSpanCap));
  }
  const int up = ok ? e[0] : 1, down = ok ? e[1] : 1, width = ok ? e[2] : 0, taps = ok ? e[3] : 0, offset = ok ? e[4] : 0,
            nblk = ok ? e[5] : resample::kMaxTile, kc = ok ? e[6] : 1;
  const int32_t word = in_lens[b];
  const int32_t n_word = word < 0 ? 0 : (word & (LASR_LEN_LEAD - 1));
  const TI* __restrict__ x = in + b * in_pitch;
  TO* __restrict__ y = out + b * out_pitch;
  const int tile = nblk * up;                      // <= kMaxTile

  if (ok && up == 1 && down == 1) {                // identity: a copy, the lead-in sample and its flag included
    const int lead = (word > 0 && (word & LASR_LEN_LEAD)) ? 1 : 0;
    int64_t n = (int64_t)n_word + lead;
    const bool whole = n <= in_pitch && n <= L_out;
    if (n > in_pitch) n = in_pitch;
    if (n > L_out) n = L_out;
    if (blockIdx.x == 0 && tid == 0) out_lens[b] = whole ? word : (int32_t)n;
    for (int64_t j0 = (int64_t)blockIdx.x * tile; j0 < L_out; j0 += (int64_t)gridDim.x * tile)
      for (int r = 0; r < kAcc; ++r) {
        const int64_t j = j0 + tid + r * kThreads;
        if (j < n) copy_sample(y + j, x + j);
        else if (j < L_out) store_sample(y + j, 0.0f);
      }
    return;
  }

  const int64_t n_in = ok ? ((int64_t)n_word < in_pitch ? (int64_t)n_word : in_pitch) : 0;
  int64_t n_out = (n_in * up + down - 1) / down;
  if (n_out > L_out) n_out = L_out;
  if (blockIdx.x == 0 && tid == 0) out_lens[b] = (int32_t)n_out;
  const float* __restrict__ hbank = reinterpret_cast<const float*>(bank) + offset;

  for (int64_t t = blockIdx.x; t * tile < L_out; t += gridDim.x) {       // every condition below is uniform over the workgroup
    const int64_t j0 = t * tile;
    if (j0 >= n_out) {                             // past the row's end: zeros up to L_out
      for (int r = 0; r < kAcc; ++r) {
        const int jl = tid + r * kThreads;
        if (jl < tile && j0 + jl < L_out) store_sample(y + j0 + jl, 0.0f);
      }
      continue;
    }
    const int64_t in0 = t * nblk * down - width;   // input index of xs[0] at tap chunk 0
    float acc[kAcc];
    int xo[kAcc], ho[kAcc];
#pragma unroll
    for (int r = 0; r < kAcc; ++r) {
      const int jl = tid + r * kThreads;
      const bool live = jl < tile && j0 + jl < n_out;
      const int q = live ? jl / up : 0;
      xo[r] = q * down;
      ho[r] = live ? jl - q * up : 0;
      acc[r] = 0.0f;
    }
    for (int k0 = 0; k0 < taps; k0 += kc) {
      const int kn = taps - k0 < kc ? taps - k0 : kc;
      const int span = (nblk - 1) * down + kn;     // <= kSpanCap by the header's construction (resample.h plan())
      __syncthreads();                             // the previous chunk / tile has been read
      for (int i = tid; i < span; i += kThreads) {
        const int64_t idx = in0 + k0 + i;
        xs[i] = (idx >= 0 && idx < n_in) ? load_sample(x + idx) : 0.0f;
      }
      __syncthreads();
      const float* __restrict__ h = hbank + (int64_t)k0 * up;
#pragma unroll 4
      for (int k = 0; k < kn; ++k) {
#pragma unroll
        for (int r = 0; r < kAcc; ++r) acc[r] = fmaf(h[k * up + ho[r]], xs[xo[r] + k], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kAcc; ++r) {
      const int jl = tid + r * kThreads;
      if (jl < tile && j0 + jl < L_out) store_sample(y + j0 + jl, j0 + jl < n_out ? acc[r] : 0.0f);
    }
  }
}

template <typename TI, typename TO>
void launch(dim3 grid, hipStream_t st, const void* bank, const void* in, int64_t in_pitch, const int32_t* in_lens, const int32_t* conv_id,
            void* out, int64_t out_pitch, int64_t L_out, int32_t* out_lens) {
  hipLaunchKernelGGL((resample_kernel<TI, TO>), grid, dim3(kThreads), 0, st, static_cast<const int32_t*>(bank), static_cast<const TI*>(in),
                     in_pitch, in_lens, conv_id, static_cast<TO*>(out), out_pitch, L_out, out_lens);
}

int host_rc(int rc, const std::string& err) { return rc == resample::kOk ? 0 : fail(LASR_E_ARG, "%s", err.c_str()); }

}  // namespace

extern "C" size_t lasr_resample_bank_bytes(const int32_t* sr_in, const int32_t* sr_out, int n_conv, int lpw, double rolloff) {
  std::string err;
  const size_t n = resample::bank_bytes(sr_in, sr_out, n_conv, lpw, rolloff, &err);
  if (!n) fail(LASR_E_ARG, "lasr_resample_bank_bytes: %s", err.c_str());
  return n;
}

extern "C" int lasr_resample_bank_write(const int32_t* sr_in, const int32_t* sr_out, int n_conv, int lpw, double rolloff, void* host_dst,
                                        size_t bytes) {
  std::string err;
  return host_rc(resample::bank_write(sr_in, sr_out, n_conv, lpw, rolloff, host_dst, bytes, &err), err);
}

extern "C" int64_t lasr_resample_out_len(int64_t n_in, int64_t up, int64_t down) {
  const int64_t n = resample::out_len(n_in, up, down);
  if (n < 0) fail(LASR_E_ARG, "lasr_resample_out_len: n_in must be >= 0 and up, down in [1, 1024]");
  return n;
}

extern "C" int64_t lasr_resample_tile(int64_t up, int64_t down, int lpw, double rolloff) {
  std::string err;
  resample::Conv c;
  if (up < 1 || down < 1 || up > resample::kMaxFactor || down > resample::kMaxFactor || resample::gcd64(up, down) != 1) {
    fail(LASR_E_ARG, "lasr_resample_tile: up and down must be coprime and in [1, 1024]");
    return -1;
  }
  if (resample::plan(down, up, lpw, rolloff, &c, &err) != resample::kOk) { fail(LASR_E_ARG, "lasr_resample_tile: %s", err.c_str()); return -1; }
  return (int64_t)c.nblk * c.up;
}

extern "C" int lasr_resample(const void* bank_dev, const void* in, int in_dtype, int64_t in_pitch, const int32_t* in_lens,
                             const int32_t* conv_id, void* out, int out_dtype, int64_t out_pitch, int64_t L_out, int32_t* out_lens,
                             int64_t B, void* stream) {
  LASR_CHECK_ARG(bank_dev && in && in_lens && out && out_lens, "lasr_resample: null pointer");
  LASR_CHECK_ARG((in_dtype == LASR_WAVE_F32 || in_dtype == LASR_WAVE_PCM16) && (out_dtype == LASR_WAVE_F32 || out_dtype == LASR_WAVE_PCM16),
                 "lasr_resample: dtypes are LASR_WAVE_F32 or LASR_WAVE_PCM16");
  LASR_CHECK_ARG(B >= 0 && in_pitch >= 0 && L_out >= 0 && out_pitch >= L_out, "lasr_resample: negative size or out_pitch < L_out");
  LASR_CHECK_SHAPE(B <= 65535 && L_out < ((int64_t)1 << 31) && in_pitch < ((int64_t)1 << 31), "lasr_resample: at most 65535 rows of fewer than 2^31 samples");
  if (B == 0) return 0;
  const int64_t tiles = (L_out + resample::kMaxTile - 1) / resample::kMaxTile;
  const dim3 grid((unsigned)(tiles < 1 ? 1 : tiles), (unsigned)B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (in_dtype == LASR_WAVE_F32 && out_dtype == LASR_WAVE_F32) launch<float, float>(grid, st, bank_dev, in, in_pitch, in_lens, conv_id, out, out_pitch, L_out, out_lens);
  else if (in_dtype == LASR_WAVE_F32) launch<float, int16_t>(grid, st, bank_dev, in, in_pitch, in_lens, conv_id, out, out_pitch, L_out, out_lens);
  else if (out_dtype == LASR_WAVE_F32) launch<int16_t, float>(grid, st, bank_dev, in, in_pitch, in_lens, conv_id, out, out_pitch, L_out, out_lens);
  else launch<int16_t, int16_t>(grid, st, bank_dev, in, in_pitch, in_lens, conv_id, out, out_pitch, L_out, out_lens);
  LASR_LAUNCH_CHECK("lasr_resample");
  return 0;
}
