// Dev microbenchmark: the 256x256 bf16 tile's K loop (gemm_bf16.hip, big_step) on v_mfma_f32_32x32x16_bf16 against
// v_mfma_f32_16x16x32_bf16 at the same 128x64 output tile per wave (8 waves, one workgroup per CU, every CU busy).
// Operands are re-read from the tile's LDS images every K step of 64 (one barrier per step, as the real loop):
//   NN: both operands K-contiguous, [256 rows][64 k] with 144-byte rows, ds_read_b128 fragments;
//   TT: both row-contiguous, [64 k][256 rows] with 576-byte rows, ds_read_b64_tr_b16 fragments
//       (SWZ: the two 32-byte halves of a 64-byte column block trade places on k-rows 8..15 of every 16);
//   NN SWZ: the 16-byte k-chunks 2j and 2j+1 trade places on rows 4..11 of every 16 (16x16x32 row reads conflict-free).
// Random bf16 data; each variant runs back to back for >= 2 s before it is timed.  Reports wall time per K step and
// the in-kernel clock, delta s_memtime / delta s_memrealtime (100 MHz), median over workgroups of the last launch.
// hipcc --offload-arch=gfx950 -O3 -o build/mfma_shape tools/micro/mfma_shape.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
union Frag { uint4 u; s16x8 s; bf16x8 b; };
typedef __attribute__((address_space(3))) s16x4 lds_s4;

static constexpr int LD_KC = 144, LDR = 576, IMG = 36864;

// 32x32x16 fragment: 8 consecutive k (ks*16 + 8*(lane>>5)) of row rb + (lane&31)
template <bool TR>
__device__ __forceinline__ bf16x8 frag32(const char* s, int rb, int ks, int lane) {
  Frag f;
  if (!TR) {
    f.u = *reinterpret_cast<const uint4*>(s + (rb + (lane & 31)) * LD_KC + ks * 32 + (lane >> 5) * 16);
  } else {
    const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const char* a0 = s + (ks * 16 + 8 * (g >> 1) + q) * LDR + (rb + 16 * (g & 1) + 4 * p) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)a0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(a0 + 4 * LDR));
    f.s = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  }
  return f.b;
}
// 16x16x32 fragment: 8 consecutive k (ks*32 + 8*(lane>>4)) of row rb + (lane&15)
template <bool TR, bool SWZ>
__device__ __forceinline__ bf16x8 frag16(const char* s, int rb, int ks, int lane) {
  Frag f;
  if (!TR) {
    const int r = lane & 15, sw = SWZ ? ((r >> 2) ^ (r >> 3)) & 1 : 0;   // SWZ: chunks trade places in pairs on rows 4..11 of every 16
    f.u = *reinterpret_cast<const uint4*>(s + (rb + r) * LD_KC + ks * 64 + ((lane >> 4) ^ sw) * 16);
  } else {
    const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const int k = ks * 32 + 8 * g + q;
    const int col = SWZ ? (rb ^ (((k >> 3) & 1) << 4)) : rb;   // rb is a multiple of 16: its 32-byte half moves
    const char* a0 = s + k * LDR + (col + 4 * p) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)a0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(a0 + 4 * LDR));
    f.s = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  }
  return f.b;
}

template <bool S16, bool TR, bool SWZ>
__global__ __launch_bounds__(512, 1) void kloop(const uint4* __restrict__ src, float* __restrict__ out, int nsteps,
                                                unsigned long long* __restrict__ clk) {
  __shared__ __attribute__((aligned(16))) char smem[2 * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 2, wn = wid & 3;
  for (int i = tid; i < 2 * IMG / 16; i += 512) reinterpret_cast<uint4*>(smem)[i] = src[(blockIdx.x * 97 + i) & 65535];
  __syncthreads();
  const char* sA = smem;
  const char* sB = smem + IMG;
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  float sum = 0.f;
  if constexpr (!S16) {
    f32x16 acc[4][2];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 2; ++j) for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int st = 0; st < nsteps; ++st) {
      bf16x8 a[2][4], b[2][2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) b[0][ni] = frag32<TR>(sB, wn * 64 + ni * 32, 0, lane);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) a[0][mi] = frag32<TR>(sA, wm * 128 + mi * 32, 0, lane);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int cur = ks & 1, nxt = cur ^ 1;
        if (ks + 1 < 4) {
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) b[nxt][ni] = frag32<TR>(sB, wn * 64 + ni * 32, ks + 1, lane);
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) a[nxt][mi] = frag32<TR>(sA, wm * 128 + mi * 32, ks + 1, lane);
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[cur][ni], a[cur][mi], acc[mi][ni], 0, 0, 0);
      }
      __syncthreads();
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 2; ++j) for (int r = 0; r < 16; ++r) sum += acc[i][j][r];
  } else {
    // groups of (2 A fragments, 8 MFMAs) over a substep's 4 B fragments; the next group's fragments are requested first
    f32x4 acc[8][4];
    for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    for (int st = 0; st < nsteps; ++st) {
      bf16x8 a[2][2], b[2][4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) b[0][ni] = frag16<TR, SWZ>(sB, wn * 64 + ni * 16, 0, lane);
#pragma unroll
      for (int h = 0; h < 2; ++h) a[0][h] = frag16<TR, SWZ>(sA, wm * 128 + h * 16, 0, lane);
#pragma unroll
      for (int gi = 0; gi < 8; ++gi) {
        const int ks = gi >> 2, mp = gi & 3, ac = gi & 1, bc = ks & 1;
        if (gi + 1 < 8) {
          const int ks1 = (gi + 1) >> 2, mp1 = (gi + 1) & 3;
          if (mp1 == 0) {
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) b[ks1 & 1][ni] = frag16<TR, SWZ>(sB, wn * 64 + ni * 16, ks1, lane);
          }
#pragma unroll
          for (int h = 0; h < 2; ++h) a[ac ^ 1][h] = frag16<TR, SWZ>(sA, wm * 128 + (2 * mp1 + h) * 16, ks1, lane);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            acc[2 * mp + h][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[bc][ni], a[ac][h], acc[2 * mp + h][ni], 0, 0, 0);
      }
      __syncthreads();
    }
    for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) for (int r = 0; r < 4; ++r) sum += acc[i][j][r];
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) { clk[2 * blockIdx.x] = c1 - c0; clk[2 * blockIdx.x + 1] = r1 - r0; }
  if (sum == 1234.5f) out[tid] = sum;   // keeps the accumulators alive; never true on this data
}

static constexpr int NWG = 256, NSTEPS = 2000;

template <bool S16, bool TR, bool SWZ>
void run(const char* name, const uint4* src, float* out, unsigned long long* dclk) {
  auto launch = [&] { hipLaunchKernelGGL((kloop<S16, TR, SWZ>), dim3(NWG), dim3(512), 0, 0, src, out, NSTEPS, dclk); };
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  float ms = 0.f;
  int n = 0;
  hipEventRecord(e0, 0);
  do {                                            // >= 2 s back to back: the clock settles under load
    for (int i = 0; i < 50; ++i) launch();
    n += 50;
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    hipEventElapsedTime(&ms, e0, e1);
  } while (ms < 2000.f);
  const int reps = 200;
  hipEventRecord(e0, 0);
  for (int i = 0; i < reps; ++i) launch();
  hipEventRecord(e1, 0);
  hipEventSynchronize(e1);
  hipEventElapsedTime(&ms, e0, e1);
  std::vector<unsigned long long> h(2 * NWG);
  hipMemcpy(h.data(), dclk, h.size() * 8, hipMemcpyDeviceToHost);
  std::vector<double> mhz(NWG), cyc(NWG);
  for (int i = 0; i < NWG; ++i) { mhz[i] = 100.0 * h[2 * i] / (double)h[2 * i + 1]; cyc[i] = h[2 * i] / (double)NSTEPS; }
  std::sort(mhz.begin(), mhz.end()); std::sort(cyc.begin(), cyc.end());
  const double us_step = ms * 1e3 / reps / NSTEPS;
  const double tflops = 2.0 * 256 * 256 * 64 * NWG / (us_step * 1e-6) / 1e12;
  printf("%-26s %8.4f us per K step  %7.1f TFLOP/s  clock %6.0f MHz  %6.0f cycles per K step  (%d warm-up launches)\n", name, us_step, tflops,
         mhz[NWG / 2], cyc[NWG / 2], n);
  fflush(stdout);
}

int main() {
  const int nsrc = 65536;
  std::vector<uint4> h(nsrc);
  srand(1234);
  for (auto& v : h) {
    uint32_t w[4];
    for (auto& x : w) {   // two random bf16 in [-1, 1)
      auto r = [] { float f = rand() / (float)RAND_MAX * 2.f - 1.f; uint32_t u; memcpy(&u, &f, 4); return u >> 16; };
      x = r() | (r() << 16);
    }
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  uint4* src; float* out; unsigned long long* clk;
  hipMalloc(&src, nsrc * 16); hipMalloc(&out, 4096); hipMalloc(&clk, 2 * NWG * 8);
  hipMemcpy(src, h.data(), nsrc * 16, hipMemcpyHostToDevice);
  for (int round = 0; round < 2; ++round) {
    run<false, false, false>("NN 32x32x16", src, out, clk);
    run<true, false, false>("NN 16x16x32", src, out, clk);
    run<true, false, true>("NN 16x16x32 swizzled", src, out, clk);
    run<false, true, false>("TT 32x32x16", src, out, clk);
    run<true, true, false>("TT 16x16x32", src, out, clk);
    run<true, true, true>("TT 16x16x32 swizzled", src, out, clk);
  }
  return hipDeviceSynchronize() != hipSuccess;
}
