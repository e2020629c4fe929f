// Pitch: a YIN F0 tracker (de Cheveigne & Kawahara 2002, steps 1-5; the definition: include/mi355tts.h), ONE launch per call.
// One workgroup of 256 threads (four waves) per frame: grid (columns, B), where the columns cover the row stride of the outputs,
// so the same launch writes the zeros behind a row's frames.  A workgroup past its row's frames writes its column's zeros and
// leaves together; the others all stay in every barrier.
//
//   stage   the frame's span x[s .. s + W + tau_max) into LDS once (wave_load_row: zeros outside the row, int16 as s * 2^-15);
//           the rest of the 3072 floats is zeroed, so every lag up to 1024 reads initialised memory.
//   d       LANES OWN LAGS: thread i owns the lags 1 + i + 256 k, k < NK = ceil(tau_max / 256) (a template argument: the
//           accumulators stay in registers).  Per step of four j: one 16-byte broadcast read of x[j .. j + 3] for all lanes and
//           all k, and per lag four reads that are consecutive across the lanes (no bank conflict).  FOUR accumulators per lag —
//           accumulator m takes the terms j = m (mod 4), j ascending, subtract then one fma — so 4 NK independent chains per
//           lane; d = (a0 + a1) + (a2 + a3).  This order is part of the definition.
//   r0      thread i sums x[j]^2 over j = i, i + 256, .. (one fma per term), wave_sum's butterfly, then (p0 + p1) + (p2 + p3).
//   c, d'   LANES OWN FOUR CONSECUTIVE LAGS 4 i + 1 .. 4 i + 4 (d is 0 behind tau_max): the thread's running sums l1 .. l4 in
//           sequence, a Hillis-Steele inclusive scan of l4 over the wave (steps 1, 2, .. 32), the waves' totals in sequence,
//           c = (wave offset + the lanes before) + l_m.  d' = c > 0 ? (d * tau) / c : 1, left in LDS over d.
//   pick    first-index reductions over the workgroup (wave butterfly by min, then the four waves), never a serial walk: the
//           first lag in [tau_min, tau_max] with d' < theta and the minimum of d' over the range in one pass; then either the
//           first lag >= it where the descent stops (tau_max, or d'(tau + 1) < d'(tau) no longer holds), or, unvoiced, the
//           first lag that holds the minimum.
//   out     thread 0: periodicity, the parabolic interpolation, f0, the level; all threads: the frame's d' row.
// LDS: 12 288 B span + 4 112 B d' + 96 B scratch = 16.5 KB a workgroup; no atomics; vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "wave_io.h"

namespace mi355tts {

constexpr int PT_THREADS = 256;
constexpr int PT_MAX_TAU = 1024;
constexpr int PT_MAX_W = 2048;
constexpr int PT_SPAN = PT_MAX_W + PT_MAX_TAU;  // 3072: the most a frame reads (window + tau_max <= 3072)

struct PitchArgs {
  const float* in_f32;  // exactly one of the two
  const short* in_i16;
  long long in_bs;      // samples between rows
  const int* samples;   // [B]
  int hop, W, tau_min, tau_max, interpolate;
  float sample_rate, theta;
  float *f0, *per, *lvl;  // [B][ld], each or null
  float* cmnd;            // [B][ld][tau_max + 1], or null
  long long ld;
};

// 256 -> 1 by min through pm[0 .. 3]; every thread gets the result (a barrier inside: uniform callers only)
__device__ __forceinline__ int pitch_block_min(int v, int* pm, int tid) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  if ((tid & 63) == 0) pm[tid >> 6] = v;
  __syncthreads();
  return min(min(pm[0], pm[1]), min(pm[2], pm[3]));
}

template <bool I16, int NK>
__global__ __launch_bounds__(PT_THREADS) void pitch_kernel(PitchArgs A) {
  __shared__ __attribute__((aligned(16))) float x[PT_SPAN];
  __shared__ float dd[PT_MAX_TAU + 4];  // d(tau), then d'(tau), at index tau
  __shared__ float sf[12];              // r0's wave sums | the scan's wave totals | the waves' minima of d'
  __shared__ int si[8];                 // the two first-index reductions
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int N = A.samples[b];
  const int tau_max = A.tau_max, W = A.W;
  const long long o = (long long)b * A.ld + t;
  float* const crow = A.cmnd ? A.cmnd + o * (tau_max + 1) : nullptr;
  if (t >= N / A.hop) {  // behind the row's frames: zeros (the whole workgroup leaves together)
    if (tid == 0) {
      if (A.f0) A.f0[o] = 0.f;
      if (A.per) A.per[o] = 0.f;
      if (A.lvl) A.lvl[o] = 0.f;
    }
    if (crow)
      for (int i = tid; i <= tau_max; i += PT_THREADS) crow[i] = 0.f;
    return;
  }
  // ---- stage
  const int s = t * A.hop - W / 2;
  const long long row = (long long)b * A.in_bs;
  const int span = W + tau_max;
  for (int i = tid; i < PT_SPAN; i += PT_THREADS) x[i] = i < span ? wave_load_row<I16>(A, row, s + i, N) : 0.f;
  __syncthreads();
  // ---- d and r0
  {
    float acc[NK][4];
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.f;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float* xl = x + tid + 1;  // lag 1 + tid + 256 k: at most 1024, so xl[256 k + j + 3] stays below x[3072]
    for (int j = 0; j < W; j += 4) {
      const float4 v = x4[j >> 2];
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const float* p = xl + 256 * k + j;
        const float e0 = v.x - p[0], e1 = v.y - p[1], e2 = v.z - p[2], e3 = v.w - p[3];
        acc[k][0] = fmaf(e0, e0, acc[k][0]);
        acc[k][1] = fmaf(e1, e1, acc[k][1]);
        acc[k][2] = fmaf(e2, e2, acc[k][2]);
        acc[k][3] = fmaf(e3, e3, acc[k][3]);
      }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int tau = 1 + tid + 256 * k;
      if (tau <= tau_max) dd[tau] = (acc[k][0] + acc[k][1]) + (acc[k][2] + acc[k][3]);
    }
    float e = 0.f;
    for (int j = tid; j < W; j += PT_THREADS) e = fmaf(x[j], x[j], e);
    e = wave_sum(e);
    if (lane == 0) sf[wave] = e;
  }
  __syncthreads();
  // ---- the prefix sum and d'
  const int tau0 = 4 * tid + 1;  // this thread's lags from here on: tau0 .. tau0 + 3
  float d[4], l[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) d[m] = tau0 + m <= tau_max ? dd[tau0 + m] : 0.f;
  l[0] = d[0];
#pragma unroll
  for (int m = 1; m < 4; ++m) l[m] = l[m - 1] + d[m];
  float inc = l[3];
#pragma unroll
  for (int st = 1; st < 64; st <<= 1) {
    const float u = __shfl_up(inc, st);
    if (lane >= st) inc += u;
  }
  float before = __shfl_up(inc, 1);
  if (lane == 0) before = 0.f;
  if (lane == 63) sf[4 + wave] = inc;
  __syncthreads();
  {
    float off = 0.f;
    for (int w = 0; w < wave; ++w) off += sf[4 + w];
    const float base = off + before;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int tau = tau0 + m;
      const float c = base + l[m];
      d[m] = c > 0.f ? (d[m] * (float)tau) / c : 1.f;
      if (tau <= tau_max) dd[tau] = d[m];
    }
    if (tid == 0) dd[0] = 1.f;
  }
  // ---- the pick: the first lag under theta and the range's minimum
  int first = INT_MAX;
  float lo = INFINITY;
#pragma unroll
  for (int m = 3; m >= 0; --m) {
    const int tau = tau0 + m;
    if (tau >= A.tau_min && tau <= tau_max) {
      if (d[m] < A.theta) first = tau;
      if (d[m] < lo) lo = d[m];
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float u = __shfl_xor(lo, m);
    lo = u < lo ? u : lo;
  }
  if (lane == 0) sf[8 + wave] = lo;
  first = pitch_block_min(first, si, tid);  // (its barrier also publishes d' and the waves' minima)
  const bool voiced = first != INT_MAX;
  if (crow)
    for (int i = tid; i <= tau_max; i += PT_THREADS) crow[i] = dd[i];
  lo = sf[8];
#pragma unroll
  for (int w = 1; w < 4; ++w) lo = sf[8 + w] < lo ? sf[8 + w] : lo;
  // ---- voiced: where the descent from `first` stops; unvoiced: the first lag that holds the minimum
  int cand = INT_MAX;
#pragma unroll
  for (int m = 3; m >= 0; --m) {
    const int tau = tau0 + m;
    if (tau < A.tau_min || tau > tau_max) continue;
    const bool stop = voiced ? tau >= first && (tau == tau_max || !(dd[tau + 1] < d[m])) : d[m] == lo;
    if (stop) cand = tau;
  }
  int taup = pitch_block_min(cand, si + 4, tid);
  if (tid != 0) return;
  if (taup == INT_MAX) taup = A.tau_min;  // (no comparison held: d' is not a number anywhere)
  const float bq = dd[taup];
  float f0 = 0.f;
  if (voiced) {
    float ts = (float)taup;
    if (A.interpolate && taup - 1 >= 1 && taup + 1 <= tau_max) {
      const float a = dd[taup - 1], c = dd[taup + 1];
      const float den = (a - 2.0f * bq) + c;
      if (den > 0.f) ts = (float)taup + (0.5f * (a - c)) / den;
    }
    f0 = A.sample_rate / ts;
  }
  if (A.f0) A.f0[o] = f0;
  if (A.per) A.per[o] = fmaxf(0.f, 1.0f - bq);
  if (A.lvl) {
    const float ms = ((sf[0] + sf[1]) + (sf[2] + sf[3])) / (float)W;
    A.lvl[o] = ms > 1e-10f ? 10.0f * log10f(ms) : -100.0f;
  }
}

}  // namespace mi355tts
