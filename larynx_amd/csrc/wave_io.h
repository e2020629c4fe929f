// What the kernels of the delivery stages (resample.h, loudness.h, limiter.h) share: a sample of an f32 or int16 row, the
// saturating int16 of a delivered sample, and the max / min of a wave and of a 256-thread workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "small_kernels.h"

namespace mi355tts {

// Sample i of the input `a` names (a stage's kernel arguments: in_f32 or in_i16, whichever form I16 says): int16 samples are
// s * 2^-15 (exact).  The caller keeps i inside the rows.
template <bool I16, class Args>
__device__ __forceinline__ float wave_load(const Args& a, long long i) {
  if constexpr (I16) return (float)a.in_i16[i] * (1.0f / 32768);
  else return a.in_f32[i];
}
// x[n] of the row that starts at `row`, zero outside [0, N); n in the caller's own width (int or long long)
template <bool I16, class Args, class Index>
__device__ __forceinline__ float wave_load_row(const Args& a, long long row, Index n, int N) {
  if (n < 0 || n >= N) return 0.f;
  return wave_load<I16>(a, row + n);
}

// the saturating int16 of a delivered sample: clamp(rintf(v * 32768), -32768, 32767)
__device__ __forceinline__ short wave_pcm(float v) { return (short)(int)fminf(fmaxf(rintf(v * 32768.0f), -32768.0f), 32767.0f); }

// 64 lanes -> 1 by max (wave_max, small_kernels.h) or min
template <bool MIN>
__device__ __forceinline__ float wave_extreme(float m) {
  if constexpr (MIN) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fminf(m, __shfl_xor(m, s));
    return m;
  } else {
    return wave_max(m);
  }
}
// the four waves' values of a 256-thread workgroup -> 1
template <bool MIN>
__device__ __forceinline__ float block_extreme_of(const float* pm) {
  return MIN ? fminf(fminf(pm[0], pm[1]), fminf(pm[2], pm[3])) : fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3]));
}
// 256 -> 1 by max or min through pm[0 .. 3]; every thread gets the result (a barrier inside: uniform callers only)
template <bool MIN>
__device__ __forceinline__ float block_extreme(float m, float* pm, int tid) {
  m = wave_extreme<MIN>(m);
  if ((tid & 63) == 0) pm[tid >> 6] = m;
  __syncthreads();
  return block_extreme_of<MIN>(pm);
}

}  // namespace mi355tts
