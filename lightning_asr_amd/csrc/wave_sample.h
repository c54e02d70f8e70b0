// One waveform sample in and out of a kernel, shared by resample.hip and wave_aug.hip: f32 as it is, PCM16 scaled by 1/32768 (exact
// in f32) on the way in and stored as clamp(rint(v * 32768), -32768, 32767) on the way out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lasr {

__device__ __forceinline__ float load_sample(const float* p) { return *p; }
__device__ __forceinline__ float load_sample(const int16_t* p) { return (float)*p * (1.0f / 32768.0f); }
__device__ __forceinline__ void store_sample(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_sample(int16_t* p, float v) {      // saturates, never wraps
  const float s = rintf(v * 32768.0f);
  *p = (int16_t)(int)fminf(fmaxf(s, -32768.0f), 32767.0f);
}
// an identity row keeps its bits when the dtypes agree; otherwise only the scale (and the rounding) applies
__device__ __forceinline__ void copy_sample(float* o, const float* i) { *o = *i; }
__device__ __forceinline__ void copy_sample(int16_t* o, const int16_t* i) { *o = *i; }
__device__ __forceinline__ void copy_sample(float* o, const int16_t* i) { *o = load_sample(i); }
__device__ __forceinline__ void copy_sample(int16_t* o, const float* i) { store_sample(o, *i); }

}  // namespace lasr
