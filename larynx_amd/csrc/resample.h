// Rational resampling by up / down with a caller-supplied symmetric prototype (include/mi355tts.h "resampling"): the delivered
// rows at another sample rate, ONE launch (TWO with MI355TTS_PCM_NORMALIZE) behind the vocoder.
//
// Output n of a row reads c = n * down + H: phase p = c mod up, newest input q = c div up, and
//   y[n] = sum over t = 0 .. Tp - 1 of table[p][t] * x[q - t]          (t ascending, one fma per term, ONE accumulator from +0)
// where table[p][t] = taps[p + t * up] (zero past the prototype: rows are Tp = T rounded up to 4 floats, T = ceil((2 H + 1) / up))
// and x is zero outside [0, N).  The padded terms and the terms outside the row add exact zeros, so the bits are those of the
// sum over the prototype's own terms in that order.
//
//   resample_kernel — a 256-thread workgroup owns 256 consecutive outputs of one row.  STAGED: their inputs span
//     q(n0 + 255) - q(n0) + Tp <= RS_SPAN samples; the workgroup stages that span, rounded up to whole rounds of 256, in LDS
//     once (int16 converted as s * 2^-15, exact, and zeros outside [0, N): the loop itself has no bounds test), requested
//     together with each lane's first table floats before the first fma; each lane then walks its own table row with 16-byte
//     loads (the table, 10-60 KB, stays in L2 for every workgroup) against LDS reads at xs[q - t].  Lanes of a wave read LDS addresses down / up apart: no conflict pattern worth
//     padding for at the ratios in use.  Not STAGED (down / up above ~7: neighbouring outputs share few inputs, the span would not
//     fit): the same loop on clamped global loads, masked afterwards.  Both forms and both input types give the same bits.
//     The launch writes the f32 row and / or the saturating int16 row (clamp(rintf(y * 32768), -32768, 32767)), zeros from the
//     row's N_out up to its stride, and — for the second launch — max |y| of every workgroup's outputs, laid out as
//     post_conv_kernel (voc_out.h) leaves them: no atomics, nothing to zero beforehand.  A tile's base position n0 * down is
//     formed in 64 bits (2^24 samples x 1024); inside the tile 32 bits are enough.
//   resample_pcm_kernel — MI355TTS_PCM_NORMALIZE: the reference's audio_float_to_int16 (larynx/audio.py:118-125) on the row's
//     N_out resampled samples, the rule and rounding of wave_out_kernel (voc_out.h): 32767 / max(0.01, peak), clip to +-32767,
//     truncate toward zero.  (wave_out_kernel itself takes a row length as frames x hop in 32 bits: N_out is neither.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_io.h"

namespace mi355tts {

constexpr int RS_TILE = 256;    // outputs per workgroup = threads
constexpr int RS_SPAN = 2048;   // staged input samples per workgroup, at most
constexpr int RS_MAX_T = 128;   // taps per phase, at most
constexpr int RS_MAX_UD = 1024; // up, down at most

struct ResampleArgs {
  const float* in_f32;  // exactly one of the two (the kernel's template parameter says which), [B][in_bs]
  const short* in_i16;
  long long in_bs;
  const int* samples;   // [B]: N per row
  const float* table;   // [up][Tp]
  int up, down, half_len, Tp;
  int stage_rounds;     // STAGED: ceil(staged span / 256), 1 .. RS_SPAN / 256
  float* y;             // optional: [B][y_bs], row = N_out samples | zeros up to y_ld
  long long y_bs, y_ld;
  short* pcm;           // optional, saturating: same layout
  long long pcm_bs, pcm_ld;
  float* peak;          // optional: max |y| of workgroup blockIdx.x at peak[b * peak_ld + blockIdx.x]
  long long peak_ld;
  const int* out_n;     // optional [B]: the row's outputs end at out_n[b] <= N_out (shift.h delivers the first n); null: all N_out
};

__device__ __forceinline__ long long resample_out_len(int N, int up, int down) { return ((long long)N * up + down - 1) / down; }

// x[i] of the row at in_row, read at a clamped address (N >= 1); the caller masks what lies outside [0, N)
template <bool I16>
__device__ __forceinline__ float resample_fetch(const ResampleArgs& a, long long in_row, int i, int N) {
  const int ic = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
  return wave_load<I16>(a, in_row + ic);
}

// xs[j] = x[lo + j] for j < 256 NE, zeros outside [0, N): NE loads per lane requested back to back, then written
template <bool I16, int NE>
__device__ __forceinline__ void resample_stage(const ResampleArgs& a, float* xs, long long in_row, int lo, int N, int tid) {
  float v[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) v[e] = resample_fetch<I16>(a, in_row, lo + tid + RS_TILE * e, N);
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int i = lo + tid + RS_TILE * e;
    xs[tid + RS_TILE * e] = (i >= 0 && i < N) ? v[e] : 0.f;
  }
}

// I16 / STAGED are template parameters, not tests inside the loop: its loads stay out of wave-uniform branches (voc_out.h:44-46);
// the staging's one branch on the launch's span holds all of a form's loads and their LDS writes, so nothing waits at its join
// that the barrier behind it would not wait for anyway
template <bool I16, bool STAGED>
__global__ __launch_bounds__(RS_TILE) void resample_kernel(const ResampleArgs a) {
  __shared__ float xs[STAGED ? RS_SPAN : 1];
  __shared__ float pm[RS_TILE / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int N = a.samples[b];
  const long long nout = a.out_n ? a.out_n[b] : resample_out_len(N, a.up, a.down);
  const long long n0 = (long long)blockIdx.x * RS_TILE, n = n0 + tid;
  float* const y = a.y ? a.y + (long long)b * a.y_bs : nullptr;
  short* const pcm = a.pcm ? a.pcm + (long long)b * a.pcm_bs : nullptr;
  if (n0 >= nout) {  // wholly in the row's tail: zeros (the whole workgroup leaves together; no peak entry is read there)
    if (y && n < a.y_ld) y[n] = 0.f;
    if (pcm && n < a.pcm_ld) pcm[n] = 0;
    return;
  }
  const long long c0 = n0 * a.down + a.half_len;  // 64 bits: n0 * down exceeds 32
  const int q0 = (int)(c0 / a.up), r0 = (int)(c0 - (long long)q0 * a.up);
  const int cl = r0 + tid * a.down;               // < 1024 + 255 * 1024
  const int dq = cl / a.up, p = cl - dq * a.up;   // this lane's newest input is q0 + dq, its phase p
  const float4* const row = reinterpret_cast<const float4*>(a.table + (long long)p * a.Tp);
  const int nt4 = a.Tp >> 2;
  const long long in_row = (long long)b * a.in_bs;
  auto fetch = [&](int i) { return resample_fetch<I16>(a, in_row, i, N); };  // (N >= 1 here)
  float4 w = row[0];
  float acc = 0.f;
  if constexpr (STAGED) {
    // xs[j] = x[lo + j], lo = q0 - (Tp - 1): the lane's term t reads xs[dq + Tp - 1 - t].  Only the span the launch's ratio
    // needs is staged: a.stage_rounds x 256 samples (1 at -> 48 000, 2 at -> 16 000, 4 at -> 8 000; the host checked that the
    // last lane's dq + Tp fits it and RS_SPAN).  One branch, uniform over the launch, holds each form's loads together.
    const int lo = q0 - (a.Tp - 1);
    if (a.stage_rounds <= 1) resample_stage<I16, 1>(a, xs, in_row, lo, N, tid);
    else if (a.stage_rounds <= 2) resample_stage<I16, 2>(a, xs, in_row, lo, N, tid);
    else if (a.stage_rounds <= 4) resample_stage<I16, 4>(a, xs, in_row, lo, N, tid);
    else resample_stage<I16, RS_SPAN / RS_TILE>(a, xs, in_row, lo, N, tid);
    __syncthreads();
    const float* xr = xs + dq + a.Tp - 1;
    for (int t4 = 0; t4 < nt4; ++t4) {
      const float4 nx = row[t4 + 1 < nt4 ? t4 + 1 : t4];
      acc = fmaf(w.x, xr[0], acc);
      acc = fmaf(w.y, xr[-1], acc);
      acc = fmaf(w.z, xr[-2], acc);
      acc = fmaf(w.w, xr[-3], acc);
      xr -= 4;
      w = nx;
    }
  } else {
    const int q = q0 + dq;
    for (int t4 = 0; t4 < nt4; ++t4) {
      const float4 nx = row[t4 + 1 < nt4 ? t4 + 1 : t4];
      const int i = q - 4 * t4;
      const float x0 = fetch(i), x1 = fetch(i - 1), x2 = fetch(i - 2), x3 = fetch(i - 3);
      acc = fmaf(w.x, (i >= 0 && i < N) ? x0 : 0.f, acc);
      acc = fmaf(w.y, (i - 1 >= 0 && i - 1 < N) ? x1 : 0.f, acc);
      acc = fmaf(w.z, (i - 2 >= 0 && i - 2 < N) ? x2 : 0.f, acc);
      acc = fmaf(w.w, (i - 3 >= 0 && i - 3 < N) ? x3 : 0.f, acc);
      w = nx;
    }
  }
  const bool live = n < nout;
  if (!live) acc = 0.f;  // the tile that holds the row's end: zeros behind it
  if (y && n < a.y_ld) y[n] = acc;
  if (pcm && n < a.pcm_ld) pcm[n] = wave_pcm(acc);
  if (a.peak) {  // (uniform per launch: the barrier is safe)
    const float m = block_extreme<false>(fabsf(acc), pm, tid);
    if (tid == 0) a.peak[(long long)b * a.peak_ld + blockIdx.x] = m;
  }
}

// y [B][y_bs] float rows of N_out samples -> out [B][o_bs] int16 rows: N_out scaled samples | zeros up to o_ld
// (out_n, optional [B]: the rows' lengths themselves, in place of N_out of samples / up / down)
__global__ __launch_bounds__(256) void resample_pcm_kernel(const float* y, long long y_bs, const int* samples, int up, int down,
                                                            const float* peak, long long peak_ld, short* out, long long o_bs,
                                                            long long o_ld, const int* out_n) {
  __shared__ float pm[4];
  const int b = blockIdx.y;
  const long long nout = out_n ? out_n[b] : resample_out_len(samples[b], up, down);
  const long long np = (nout + RS_TILE - 1) / RS_TILE;
  float m = 0.f;
  for (long long i = threadIdx.x; i < np; i += blockDim.x) m = fmaxf(m, peak[(long long)b * peak_ld + i]);
  const float g = 32767.0f / fmaxf(0.01f, block_extreme<false>(m, pm, threadIdx.x));
  const float* src = y + (long long)b * y_bs;
  short* dst = out + (long long)b * o_bs;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < o_ld; i += step) {
    short s = 0;
    if (i < nout) s = (short)(int)fminf(fmaxf(src[i] * g, -32767.0f), 32767.0f);
    dst[i] = s;
  }
}

}  // namespace mi355tts
