// Pitch shift and tempo: a period-synchronous overlap-add stretch by up / down (the definition: include/mi355tts.h "pitch shift"),
// TWO kernels between pitch_kernel (pitch.h: the periods) and resample_kernel (resample.h: the stretch played back faster or slower).
// Time domain throughout: no transcendental function, no atomics, vector stores only.
//
//   shift_mark_kernel — the read positions s_k of every row, ONE WAVE per row.  The recurrence s_k = a_k + (e - rint(rint(e / T) T)),
//     e = s_(k-1) + Hs - a_k, is serial in k; everything around it is not.  Per round of 64 frames: lane i forms c_k, a_k and the
//     pitch frame j of frame k0 + i, loads f0[j] (the 64 loads of a round are independent of the chain and in flight together) and
//     divides T = fs / f0 (T = 0 marks an unvoiced frame); a_k and T go to LDS; then the chain of the round runs over the 64 LDS
//     entries (broadcast reads; one division, two rintf, one product per step, all f32, nothing fused: the product feeds rintf,
//     not an add), its s_k go to LDS and leave with one coalesced store.  The lanes also write the zeros behind the row's K.
//   shift_ola_kernel — y[t] = rn(rn(w[i1] x[s_k1 + i1]) + rn(w[i2] x[s_(k1+1) + i2])): a 256-thread workgroup owns 1024 consecutive
//     outputs, a thread FOUR consecutive ones, so a wave owns the 256 outputs of one resample-tile and leaves their max |y| where
//     resample_pcm_kernel (resample.h) expects it, with no barrier.  Hs a multiple of 4 (N a multiple of 8): the four share their
//     two frames, the window comes in two 16-byte loads and the positions in two loads per thread; else each output finds its own.
//     The samples are read one by one: s_k has any parity, so x[s_k + i] is 16-byte aligned for one thread in four at best, and
//     the rows' ends are masked per sample (shift_x: clamped loads, no branch).  The float row leaves in 16-byte stores where its base allows.
//     Two products and one add, each rounded by itself: shift_mul / shift_add keep the compiler from contracting them (HIP's
//     __fmul_rn is a plain product that the fp-contract default may fuse), so numpy states this stage bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_io.h"

namespace mi355tts {

constexpr int SH_THREADS = 256;
constexpr int SH_PER_THREAD = 4;
constexpr int SH_TILE = SH_THREADS * SH_PER_THREAD;  // outputs per workgroup
constexpr int SH_PEAK_TILE = 64 * SH_PER_THREAD;     // outputs per wave = RS_TILE of resample.h (shift_forward.h asserts it)
constexpr int SH_MAX_UD = 64;
constexpr int SH_MAX_N = 2048;

struct ShiftMarkArgs {
  const int* samples;  // [B]
  const float* f0;     // [B][f0_bs] of pitch_kernel, or null: no row has a pitch frame
  long long f0_bs;
  int hop_p;
  float sample_rate;
  int up, down, Hs;
  int* pos;            // [B][pos_bs]: K positions | zeros up to pos_ld
  long long pos_bs, pos_ld;
};

struct ShiftOlaArgs {
  const float* in_f32;  // exactly one of the two
  const short* in_i16;
  long long in_bs;
  const int* samples;   // [B]
  const float* win;     // [2 Hs]
  int up, down, Hs;
  const int* pos;       // [B][pos_bs]
  long long pos_bs;
  float* y;             // optional: [B][y_bs], row = L samples | zeros up to y_ld
  long long y_bs, y_ld;
  short* pcm;           // optional, saturating: same layout
  long long pcm_bs, pcm_ld;
  float* peak;          // optional: max |y| of outputs [256 i, 256 i + 256) at peak[b * peak_ld + i], i < peak_ld
  long long peak_ld;
};

// L = ceil(n up / down): n <= 2^24 and up <= 64, so 32 bits hold it (a 64-bit division costs a hundred instructions)
__device__ __forceinline__ long long shift_len(int n, int up, int down) { return ((unsigned)n * (unsigned)up + (unsigned)(down - 1)) / (unsigned)down; }

// one correctly rounded f32 product / sum, never contracted into an fma with its neighbour
__device__ __forceinline__ float shift_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float shift_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// x[i] of a row of n >= 1 samples, zero outside [0, n): loaded at a clamped address and masked afterwards, so the loads of a
// thread are all requested before the first is used (no branch around a load)
template <bool I16>
__device__ __forceinline__ float shift_x(const ShiftOlaArgs& a, long long row, long long i, int n) {
  const long long ic = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  const float v = wave_load<I16>(a, row + ic);
  return i == ic ? v : 0.f;
}

__global__ __launch_bounds__(64) void shift_mark_kernel(const ShiftMarkArgs a) {
  __shared__ int sa[64];
  __shared__ float sT[64];
  __shared__ int ss[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = a.samples[b], Hs = a.Hs;
  const long long L = shift_len(n, a.up, a.down);
  const long long K = L > 0 ? (L - 1) / Hs + 2 : 0;
  const int Fp = a.f0 ? n / a.hop_p : 0;
  const float* const f0 = a.f0 ? a.f0 + (long long)b * a.f0_bs : nullptr;
  int* const pos = a.pos + (long long)b * a.pos_bs;
  int s = 0;
  for (long long k0 = 0; k0 < K; k0 += 64) {
    const long long k = k0 + lane;
    int ak = 0;
    float T = 0.f;  // 0: s_k = a_k (frame 0, an unvoiced frame, a row without pitch frames)
    if (k < K) {
      const long long c = k * Hs * a.down / a.up;  // < 2^37
      ak = (int)c - Hs;
      if (k >= 1 && Fp > 0) {
        const long long j = (c + a.hop_p / 2) / a.hop_p;
        const float f = f0[j < Fp - 1 ? j : Fp - 1];
        if (f != 0.f) T = a.sample_rate / f;
      }
    }
    sa[lane] = ak;
    sT[lane] = T;
    __syncthreads();
    const int cnt = K - k0 < 64 ? (int)(K - k0) : 64;
    if (lane == 0) {
      for (int i = 0; i < cnt; ++i) {
        const int ai = sa[i];
        const float Ti = sT[i];
        if (Ti == 0.f) {
          s = ai;
        } else {
          const int e = (s + Hs) - ai;
          const float q = rintf((float)e / Ti);
          const float m = rintf(shift_mul(q, Ti));
          s = ai + (e - (int)m);
        }
        ss[i] = s;
      }
    }
    __syncthreads();
    if (k < K) pos[k] = ss[lane];
    s = ss[cnt - 1];  // (every lane: lane 0 carries it into the next round)
    __syncthreads();
  }
  for (long long k = K + lane; k < a.pos_ld; k += 64) pos[k] = 0;
}

template <bool I16>
__global__ __launch_bounds__(SH_THREADS) void shift_ola_kernel(const ShiftOlaArgs a) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = a.samples[b], Hs = a.Hs;
  const long long L = shift_len(n, a.up, a.down);
  const long long t0 = ((long long)blockIdx.x * SH_THREADS + tid) * SH_PER_THREAD;
  const long long row = (long long)b * a.in_bs;
  const int* const pos = a.pos + (long long)b * a.pos_bs;
  float v[SH_PER_THREAD] = {0.f, 0.f, 0.f, 0.f};
  if ((Hs & 3) == 0 && t0 + SH_PER_THREAD <= L) {  // the four outputs share their frames k1 and k1 + 1 (<= K - 1)
    const unsigned k1 = (unsigned)t0 / (unsigned)Hs;  // t0 < L <= 2^30
    const int i2 = (int)((unsigned)t0 - k1 * (unsigned)Hs), i1 = i2 + Hs;
    const long long s1 = pos[k1], s2 = pos[k1 + 1];
    const float4 wa = *reinterpret_cast<const float4*>(a.win + i1), wb = *reinterpret_cast<const float4*>(a.win + i2);
    const float w1[4] = {wa.x, wa.y, wa.z, wa.w}, w2[4] = {wb.x, wb.y, wb.z, wb.w};
    float x1[4], x2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x1[e] = shift_x<I16>(a, row, s1 + i1 + e, n);
      x2[e] = shift_x<I16>(a, row, s2 + i2 + e, n);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = shift_add(shift_mul(w1[e], x1[e]), shift_mul(w2[e], x2[e]));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long t = t0 + e;
      if (t < L) {
        const unsigned k1 = (unsigned)t / (unsigned)Hs;
        const int i2 = (int)((unsigned)t - k1 * (unsigned)Hs), i1 = i2 + Hs;
        const float xa = shift_x<I16>(a, row, (long long)pos[k1] + i1, n);
        const float xb = shift_x<I16>(a, row, (long long)pos[k1 + 1] + i2, n);
        v[e] = shift_add(shift_mul(a.win[i1], xa), shift_mul(a.win[i2], xb));
      }
    }
  }
  if (a.y) {
    float* const y = a.y + (long long)b * a.y_bs;
    if ((reinterpret_cast<uintptr_t>(y) & 15) == 0 && t0 + SH_PER_THREAD <= a.y_ld) {
      *reinterpret_cast<float4*>(y + t0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (t0 + e < a.y_ld) y[t0 + e] = v[e];
    }
  }
  if (a.pcm) {
    short* const pcm = a.pcm + (long long)b * a.pcm_bs;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (t0 + e < a.pcm_ld) pcm[t0 + e] = wave_pcm(v[e]);
  }
  if (a.peak) {  // (uniform per launch)
    const float m = wave_extreme<false>(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    const long long i = (long long)blockIdx.x * (SH_THREADS / 64) + (tid >> 6);
    if ((tid & 63) == 0 && i < a.peak_ld) a.peak[(long long)b * a.peak_ld + i] = m;
  }
}

}  // namespace mi355tts
