// Forced alignment (mi355tts_glow_align): the kernels around the forward flow — squeeze in, unsqueeze out, the un-fused forms
// of the forward ActNorm / InvConvNear / coupling (the fused form is glow_fwd_kernel, coltile.h) — the score matrix and the
// best monotonic path.
//
//   logp[t][j] = -0.5 M ln(2 pi) - 0.5 sum_c z[c][j]^2 + sum_c x_m[c][t] z[c][j] - 0.5 sum_c x_m[c][t]^2
//     Glow-TTS's likelihood of frame j under id t's Gaussian with x_logs = 0 (mean_only voices), written TIME-MAJOR [F][ldp] so
//     that one step of the path recurrence reads contiguous memory.
//   path: glow_tts/utils.py:59-96 (maximum_path) in float32 — one max and one add per cell, so v is numpy's bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "prio.h"

namespace mi355tts {

// G13 backwards: [M][F] -> the squeezed [n M][F / n] (glow_tts/utils.py:135-147), masked to the row's F (a multiple of n);
// columns [F / n, z_ld) are zero-filled
__global__ void mel_squeeze_kernel(const float* mel, long long mel_bs, int mel_ld, const int* frames, int M, int n_sqz, float* z,
                                   long long z_bs, int z_ld) {
  GLOW_PRIO();
  const int b = blockIdx.z;
  const int F = frames[b];
  const int j2 = blockIdx.x * blockDim.x + threadIdx.x;
  if (j2 >= z_ld) return;
  for (int c = blockIdx.y; c < M; c += gridDim.y)
    for (int s = 0; s < n_sqz; ++s) {
      const int j = j2 * n_sqz + s;
      z[(long long)b * z_bs + (long long)(s * M + c) * z_ld + j2] = j < F ? mel[(long long)b * mel_bs + (long long)c * mel_ld + j] : 0.f;
    }
}

// unsqueeze (utils.py:150-160): [n M][F / n] -> [M][out_ld], zero past the row's F
__global__ void z_unsqueeze_kernel(const float* x, long long x_bs, int x_ld, const int* frames, int M, int n_sqz, float* out,
                                   long long out_bs, int out_ld) {
  GLOW_PRIO();
  const int b = blockIdx.z;
  const int F = frames[b];
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= out_ld) return;
  const int s = j % n_sqz, j2 = j / n_sqz;
  for (int c = blockIdx.y; c < M; c += gridDim.y)
    out[(long long)b * out_bs + (long long)c * out_ld + j] = j < F ? x[(long long)b * x_bs + (long long)(s * M + c) * x_ld + j2] : 0.f;
}

// ActNorm forward (layers.py:196) followed by InvConvNear forward (layers.py:247-272, `w` = the forward n x n weight), in place
// on x[B][C][ld]: invconv_actnorm_kernel's inverse, same channel groups
__global__ void actnorm_invconv_fwd_kernel(float* x, long long bs, int ld, const int* len, int C, int ns, const float* w,
                                           const float* an_bias, const float* an_escale) {
  const int b = blockIdx.z;
  const int T = len[b];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int groups = C / ns;
  const int hs = ns / 2;
  float* xb = x + (long long)b * bs + t;
  for (int k = blockIdx.y; k < groups; k += gridDim.y) {
    float in[8], o[8];
    for (int n = 0; n < ns; ++n) {
      const int a = n / hs, s = n - a * hs;
      const int c = a * (C / 2) + k * hs + s;
      in[n] = an_bias[c] + an_escale[c] * xb[(long long)c * ld];
    }
    for (int m = 0; m < ns; ++m) {
      float acc = 0.f;
      for (int n = 0; n < ns; ++n) acc += w[m * ns + n] * in[n];
      o[m] = acc;
    }
    for (int m = 0; m < ns; ++m) {
      const int a = m / hs, s = m - a * hs;
      xb[(long long)(a * (C / 2) + k * hs + s) * ld] = o[m];
    }
  }
}

// coupling forward (attentions.py:138): z1 = m + exp(logs) * x1 with ml = end(wn_out) [B][2 half][ld] (m rows, then logs)
__global__ void coupling_fwd_kernel(float* z, const float* ml, long long bs, int ld, const int* len, int half) {
  const int b = blockIdx.z;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= len[b]) return;
  for (int c = blockIdx.y; c < half; c += gridDim.y) {
    const long long o = (long long)b * bs + (long long)c * ld + t;
    float* z1 = z + o + (long long)half * ld;
    *z1 = ml[o] + expf(ml[o + (long long)half * ld]) * *z1;
  }
}

// ---- scores.  A workgroup computes 64 ids x SC_TJ frames; every sum runs over c = 0 .. M - 1 in ascending order, one fmaf per
// term, whatever the tiling or the batch: a row of a batch gets the bits of its solo call.  Ids [P, ldp) are written as 0 (the
// path kernel reads whole rows; what it computes from them never reaches an id < P).
constexpr int SC_TJ = 16;
constexpr int SC_MAXM = 256;
__global__ __launch_bounds__(256) void align_score_kernel(const float* xm, long long xm_bs, int xm_ld, const int* lens, const float* z,
                                                          long long z_bs, int z_ld, const int* frames, int M, float c0, float* logp,
                                                          long long lp_bs, int ldp) {
  __shared__ float zs[SC_MAXM][SC_TJ];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int P = lens[b], F = frames[b];
  const int j0 = blockIdx.y * SC_TJ;
  if (j0 >= F) return;
  const float* zb = z + (long long)b * z_bs;
  for (int e = tid; e < M * SC_TJ; e += 256) {
    const int c = e / SC_TJ, jj = e % SC_TJ;
    zs[c][jj] = j0 + jj < F ? zb[(long long)c * z_ld + j0 + jj] : 0.f;
  }
  __syncthreads();
  const int t = blockIdx.x * 64 + (tid & 63), ty = tid >> 6;
  const float* xp = xm + (long long)b * xm_bs + (t < P ? t : P - 1);
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, zz[4] = {0.f, 0.f, 0.f, 0.f}, xx = 0.f;
  for (int c = 0; c < M; ++c) {
    const float x = xp[(long long)c * xm_ld];
    xx = fmaf(x, x, xx);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float zv = zs[c][ty * 4 + i];
      acc[i] = fmaf(x, zv, acc[i]);
      zz[i] = fmaf(zv, zv, zz[i]);
    }
  }
  float* lp = logp + (long long)b * lp_bs;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = j0 + ty * 4 + i;
    if (j < F) lp[(long long)j * ldp + t] = t < P ? ((c0 - 0.5f * zz[i]) + acc[i]) - 0.5f * xx : 0.f;
  }
}

// mi355tts_op_maximum_path's way in: the reference's [B][P_ld][F_ld] -> time-major [B][Fmax][ldp], 0 outside a row's P x F
__global__ void path_transpose_kernel(const float* value, int P_ld, int F_ld, const int* lens, const int* frames, float* logp,
                                      long long lp_bs, int ldp, int Fmax) {
  const int b = blockIdx.z, j = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ldp || j >= Fmax) return;
  const bool in = t < lens[b] && j < frames[b];
  logp[(long long)b * lp_bs + (long long)j * ldp + t] = in ? value[((long long)b * P_ld + t) * F_ld + j] : 0.f;
}

// ---- the best monotonic path.  The sweep is sequential in j and parallel in t: ONE wave per row (no barrier in the sweep),
// lane l holds v of the ids [CH l, CH l + CH) in registers, the left neighbour's last v comes by __shfl_up, and the rows of logp
// are requested PATH_D frames ahead (the loads do not depend on v).  Direction bits ("stay") are packed 32 ids per word, 2 CH
// words per frame: in LDS when the row's F frames fit PATH_LDS_WORDS, else in global memory, from where the backtrack stages
// them through LDS in blocks of frames and walks each block there (one dependent LDS read per frame, never a global one).
constexpr int PATH_MAX_P = 2048;
constexpr int PATH_LDS_WORDS = 24576;  // 96 KB
template <int CH>
struct PathCfg {
  static constexpr int W = 2 * CH;                               // words of direction bits per frame
  static constexpr int D = CH >= 32 ? 1 : (CH <= 4 ? 8 : 32 / CH);  // frames in flight
};

template <int CH>
__device__ __forceinline__ void path_load_row(const float* p, float (&r)[CH]) {
  if constexpr (CH >= 4) {
#pragma unroll
    for (int i = 0; i < CH / 4; ++i) {
      const float4 v = reinterpret_cast<const float4*>(p)[i];
      r[4 * i] = v.x;
      r[4 * i + 1] = v.y;
      r[4 * i + 2] = v.z;
      r[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < CH; ++i) r[i] = p[i];
  }
}

// lane 0 walks frames [jlo, jhi) backwards over the bits of those frames at `bits` (frame jlo first)
template <int W>
__device__ __forceinline__ void path_walk(const unsigned* bits, int jlo, int jhi, int& idx, int& run, int* ldur) {
  for (int j = jhi - 1; j >= jlo; --j) {
    const unsigned word = bits[(j - jlo) * W + (idx >> 5)];
    const bool stay = (word >> (idx & 31)) & 1u;
    ++run;
    if (!stay && idx > 0) {  // (id 0 always stays: its left neighbour is -inf)
      ldur[idx] = run;
      run = 0;
      --idx;
    }
  }
}

template <int CH>
__global__ __launch_bounds__(64) void align_path_kernel(const float* logp, long long lp_bs, int ldp, const int* lens, const int* frames,
                                                       unsigned* gbits, long long gb_bs, int* dur, int dur_ld, float* score) {
  constexpr int W = PathCfg<CH>::W, D = PathCfg<CH>::D;
  __shared__ unsigned lbits[PATH_LDS_WORDS];
  __shared__ int ldur[PATH_MAX_P];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int P = lens[b], F = frames[b];
  const bool in_lds = (long long)F * W <= PATH_LDS_WORDS;
  unsigned* gb = gbits + (long long)b * gb_bs;
  unsigned* dst = in_lds ? lbits : gb;
  const float* lp = logp + (long long)b * lp_bs + lane * CH;
  const int t0 = lane * CH;
  const int wshift = (lane * CH) & 31, widx = (lane * CH) >> 5;
  const float ninf = -INFINITY;
  float v[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) v[i] = 0.f;
  float cur[D][CH], nxt[D][CH];
#pragma unroll
  for (int d = 0; d < D; ++d) path_load_row<CH>(lp + (long long)(d < F ? d : F - 1) * ldp, cur[d]);
  for (int jb = 0; jb < F; jb += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int j = jb + D + d;
      path_load_row<CH>(lp + (long long)(j < F ? j : F - 1) * ldp, nxt[d]);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int j = jb + d;
      if (j < F) {  // uniform over the wave
        float left = __shfl_up(v[CH - 1], 1);
        if (lane == 0) left = ninf;
        unsigned bits = 0;
#pragma unroll
        for (int i = CH - 1; i >= 0; --i) {  // downwards: v[i - 1] is still the previous frame's
          const float v0 = i > 0 ? v[i - 1] : left;
          const bool stay = v[i] >= v0;  // a tie stays
          const float m = stay ? v[i] : v0;
          v[i] = t0 + i <= j ? m + cur[d][i] : ninf;
          bits |= (stay ? 1u : 0u) << i;
        }
        unsigned word = bits << wshift;
#pragma unroll
        for (int m = 1; m < 32 / CH; m <<= 1) word |= __shfl_xor(word, m);
        if (wshift == 0) dst[(long long)j * W + widx] = word;
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
      for (int i = 0; i < CH; ++i) cur[d][i] = nxt[d][i];
  }
#pragma unroll
  for (int i = 0; i < CH; ++i)
    if (t0 + i == P - 1) score[b] = v[i];
  for (int t = lane; t < P; t += 64) ldur[t] = 0;
  __syncthreads();
  int idx = P - 1, run = 0;
  if (in_lds) {
    if (lane == 0) path_walk<W>(lbits, 0, F, idx, run, ldur);
  } else {
    const int FB = PATH_LDS_WORDS / W;
    for (int jhi = F; jhi > 0; jhi -= FB) {
      const int jlo = jhi > FB ? jhi - FB : 0;
      for (int e = lane; e < (jhi - jlo) * W; e += 64) lbits[e] = gb[(long long)jlo * W + e];
      __syncthreads();
      if (lane == 0) path_walk<W>(lbits, jlo, jhi, idx, run, ldur);
      __syncthreads();
    }
  }
  if (lane == 0) ldur[idx] = run;
  __syncthreads();
  int* db = dur + (long long)b * dur_ld;
  for (int t = lane; t < dur_ld; t += 64) db[t] = t < P ? ldur[t] : 0;
}

}  // namespace mi355tts
