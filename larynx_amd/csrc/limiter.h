// True-peak meter (ITU-R BS.1770-4 Annex 2) and look-ahead limiter of delivered rows (include/mi355tts.h "limiter"):
// TWO launches meter a row, SIX limit it, whatever N and B are.
//
// Per row x[0 .. N), gain G, ceiling C, oversampling os, look-ahead la, release a, window w[la + 1] (the definition and its
// arithmetic: the header).  The row's positions j = k + la, k = -la .. N - 1, are what the hold and the release run over:
// Np = N + la of them, position j holding step k = j - la.
//   limiter_peak_kernel    a workgroup owns LM_TILE = 256 samples: their inputs (256 + Tp - 1 + (os - 1 + H) div os <= 447
//                          samples, int16 converted as s * 2^-15, zeros outside the row) staged in LDS once; lane n walks the os
//                          polyphase rows (the phase is the same for every lane: the table is read at wave-uniform addresses)
//                          with the term order of resample_kernel at up = os, down = 1, keeps tp[n] = max(|x[n]|, |u[n os + p]|),
//                          writes c[n] = tp G <= C ? 1 : C / (tp G) (not in a meter call) and the tile's max tp.
//   limiter_reduce_kernel  one workgroup per row: the max of its tiles' peaks (TP), or — second use, behind the apply kernel —
//                          the min of its tiles' smallest gains.
//   limiter_hold_kernel    a workgroup owns a GROUP of LM_GROUP = 4096 positions, a thread a CHUNK of LM_CHUNK = 16.  c over the
//                          group's windows (4096 + la + 1 values, 1 outside the row) staged in LDS once; log2 rounds of
//                          in-place doubling (M_2j[i] = min(M_j[i], M_j[i + j]), every lane's values read into registers before
//                          any is written) leave the minimum over P = the largest power of two <= la + 2 values, and
//                          m[k] = min(c[k - 1 .. k + la]) is the min of two of those.  The release d[k] = max(1 - m[k], a d[k-1])
//                          is the one recurrence, and its operator (max, x a^len) is associative: every chunk runs from d = 0,
//                          the chunks' end states are scanned inside the workgroup (Hillis-Steele, 8 rounds, round j takes
//                          a^(16 2^j) times the state 2^j chunks back), every chunk is resolved from the scanned end state of
//                          the chunk before it: the depth of every position for a group that itself starts from d = 0, and the
//                          group's end state.
//   limiter_carry_kernel   one workgroup per row: the groups' end states from LDS, D_g = max(Z_g, a^4096 D_(g-1)), in sequence
//                          (a row has at most 4097 groups).
//   limiter_apply_kernel   a workgroup owns 256 samples: the depths of positions n0 .. n0 + 255 + la, each resolved from its
//                          group's true start state (max(d, a^(i + 1) D_(g-1)), i the position inside the group), staged in LDS
//                          once; s[n] = max(0, 1 - sum_j w[j] d[n - j]) (the window at wave-uniform addresses, the depths at
//                          consecutive LDS addresses: no bank conflict), the curve, y = clamp((x G) s, +-C), the saturating int16,
//                          zeros up to the rows' strides, and the tile's smallest s.
// The powers a^0 .. a^4096 are computed on the host in double at load time, rounded to f32 once and passed as data
// (LimiterArgs::pw).  With a = 0 every power but the first is 0 and every step above is the sequential f32 definition bit for bit;
// with a > 0 the carried terms see FEWER roundings than the sequential product a (a (a ...)).  No atomics: every max, min and sum
// is ordered by the row alone, not by the grid or B.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_io.h"

namespace mi355tts {

constexpr int LM_TILE = 256;                      // samples per workgroup of the peak and apply kernels = threads
constexpr int LM_THREADS = 256;                   // chunks per workgroup of the hold kernel
constexpr int LM_CHUNK = 16;                      // positions per thread
constexpr int LM_GROUP = LM_CHUNK * LM_THREADS;   // positions per workgroup
constexpr int LM_ROW = LM_CHUNK + 1;              // a chunk's stride in LDS: lane t walks bank 17 t + i
constexpr int LM_MAX_OS = 8;
constexpr int LM_MAX_T = 128;                     // taps per phase, at most
constexpr int LM_MAX_LA = 1024;
constexpr int LM_XSPAN = 512;                     // staged inputs of a peak tile: 256 + 127 + 64 at most
constexpr int LM_STAGE_ROUNDS = (LM_GROUP + LM_MAX_LA + 1 + LM_THREADS - 1) / LM_THREADS;  // 21 rounds of 256 staged c values
constexpr int LM_DSPAN = LM_TILE + LM_MAX_LA;     // staged depths of an apply tile
constexpr int LM_MAX_GROUPS = ((1 << 24) + LM_MAX_LA + LM_GROUP - 1) / LM_GROUP;  // 4097
static_assert(LM_TILE - 1 + (LM_MAX_T - 1) + ((LM_MAX_OS - 1) + (LM_MAX_T * LM_MAX_OS - 1) / 2) / LM_MAX_OS < LM_XSPAN, "peak tile span");

struct LimiterArgs {
  const float* in_f32;  // exactly one of the two (a template parameter says which), [B][in_bs]
  const short* in_i16;
  long long in_bs;
  const int* samples;   // [B]
  const float* gain;    // [B]: G
  float ceiling;
  int os, half_len, Tp; // Tp: floats per polyphase row (1 with os = 1: no table)
  const float* table;   // [os][Tp]
  int la;
  const float* win;     // [la + 1]
  const float* pw;      // [LM_GROUP + 1]: a^k
  float* c;             // [B][c_bs]: the required gain per sample; null in a meter call
  long long c_bs;
  float* tpeak;         // [B][t_ld]: max tp of every tile
  float* tmin;          // [B][t_ld]: min s of every tile
  long long t_ld;
  float* dg;            // [B][gmax * LM_GROUP]: the depth of every position of a group that starts from 0
  float* gs;            // [B][gmax]: the group's end state Z_g, then its TRUE end state D_g
  int gmax;
  float* res;           // [B][2]: TP, min s
  float* y;             // optional outputs, rows [B][*_bs]: N values | zeros up to *_ld
  long long y_bs, y_ld;
  short* pcm;
  long long pcm_bs, pcm_ld;
  float* curve;
  long long curve_bs, curve_ld;
};

template <bool I16>
__global__ __launch_bounds__(LM_TILE) void limiter_peak_kernel(const LimiterArgs a) {
  __shared__ float xs[LM_XSPAN];
  __shared__ float pm[LM_TILE / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int N = a.samples[b];
  const int n0 = (int)blockIdx.x * LM_TILE, n = n0 + tid;
  if (n0 >= N) return;  // (the whole workgroup: nothing reads this tile's entries)
  const long long row = (long long)b * a.in_bs;
  // xs[i] = x[lo + i], lo = n0 - (Tp - 1): term t of the lane's phase p reads xs[tid + dq(p) + Tp - 1 - t]
  const int lo = n0 - (a.Tp - 1);
#pragma unroll
  for (int e = 0; e < LM_XSPAN / LM_TILE; ++e) xs[tid + LM_TILE * e] = wave_load_row<I16>(a, row, lo + tid + LM_TILE * e, N);
  __syncthreads();
  float tp = fabsf(xs[tid + a.Tp - 1]);
  if (a.os > 1) {
    for (int p = 0; p < a.os; ++p) {  // u[n os + p]: c = n os + p + H, newest input n + (p + H) div os, phase (p + H) mod os
      const int cp = p + a.half_len, dq = cp / a.os, ph = cp - dq * a.os;
      const float* trow = a.table + ph * a.Tp;
      const float* xr = xs + tid + dq + a.Tp - 1;
      float acc = 0.f;
      for (int t = 0; t < a.Tp; ++t) acc = fmaf(trow[t], xr[-t], acc);
      tp = fmaxf(tp, fabsf(acc));
    }
  }
  if (n >= N) tp = 0.f;
  if (a.c && n < N) {
    const float t = tp * a.gain[b];
    a.c[(long long)b * a.c_bs + n] = t <= a.ceiling ? 1.f : a.ceiling / t;
  }
  const float m = block_extreme<false>(tp, pm, tid);
  if (tid == 0) a.tpeak[(long long)b * a.t_ld + blockIdx.x] = m;
}

// res[b][MIN] = the max of the row's tile peaks (from 0), or the min of its tiles' smallest gains (from 1)
template <bool MIN>
__global__ __launch_bounds__(LM_THREADS) void limiter_reduce_kernel(const LimiterArgs a) {
  __shared__ float pm[LM_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = a.samples[b];
  const int tiles = (N + LM_TILE - 1) / LM_TILE;  // <= t_ld
  const float* src = (MIN ? a.tmin : a.tpeak) + (long long)b * a.t_ld;
  float m = MIN ? 1.f : 0.f;
  for (int i = tid; i < tiles; i += LM_THREADS) m = MIN ? fminf(m, src[i]) : fmaxf(m, src[i]);
  m = block_extreme<MIN>(m, pm, tid);
  if (tid == 0) a.res[2 * b + (MIN ? 1 : 0)] = m;
}

__global__ __launch_bounds__(LM_THREADS) void limiter_hold_kernel(const LimiterArgs a) {
  __shared__ float cs[LM_STAGE_ROUNDS * LM_THREADS];
  __shared__ float es[LM_THREADS * LM_ROW];
  __shared__ float st[2][LM_THREADS];
  const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const int N = a.samples[b];
  const int j0 = g * LM_GROUP;
  if (N == 0 || j0 >= N + a.la) return;  // (the whole workgroup: nothing reads this group's entries)
  const float* c = a.c + (long long)b * a.c_bs;
  const int W = a.la + 2;                        // the hold's window: c[k - 1 .. k + la]
  const int rounds = (LM_GROUP + a.la + 1 + LM_THREADS - 1) / LM_THREADS;  // <= LM_STAGE_ROUNDS
  const int staged = rounds * LM_THREADS;
  // cs[i] = c[j0 - la - 1 + i] (1 outside the row): position j0 + q holds step k = j0 + q - la, whose window starts at cs[q]
  for (int e = 0; e < rounds; ++e) {
    const int i = tid + LM_THREADS * e, n = j0 - a.la - 1 + i;
    cs[i] = (n >= 0 && n < N) ? c[n] : 1.f;
  }
  __syncthreads();
  int P = 1;
  for (; 2 * P <= W; P *= 2) {  // cs[i]: the min of P values from i on -> of 2 P (a partner past the staged span: the value itself)
    float v[LM_STAGE_ROUNDS];
#pragma unroll
    for (int e = 0; e < LM_STAGE_ROUNDS; ++e) {
      const int i = tid + LM_THREADS * e;
      v[e] = e < rounds ? fminf(cs[i], cs[i + P < staged ? i + P : i]) : 1.f;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < LM_STAGE_ROUNDS; ++e)
      if (e < rounds) cs[tid + LM_THREADS * e] = v[e];
    __syncthreads();
  }
  // 1 - m of position j0 + q into its chunk's padded row (q + W - P <= 4095 + la + 1 < staged)
#pragma unroll
  for (int e = 0; e < LM_CHUNK; ++e) {
    const int q = tid + LM_THREADS * e;
    es[(q >> 4) * LM_ROW + (q & 15)] = 1.f - fminf(cs[q], cs[q + W - P]);
  }
  static_assert(LM_CHUNK == 16, "q >> 4, q & 15");
  __syncthreads();
  float* ec = es + tid * LM_ROW;
  const float a1 = a.pw[1];
  float dl[LM_CHUNK];
  float d = 0.f;
#pragma unroll
  for (int i = 0; i < LM_CHUNK; ++i) {
    d = fmaxf(ec[i], a1 * d);
    dl[i] = d;
  }
  float s = d;
  int cur = 0;
  st[0][tid] = s;
  __syncthreads();
  for (int j = 0; j < 8; ++j) {  // after round j: s_k = max over the last 2^(j+1) chunks i <= k of a^(16 (k - i)) z_i
    const int dd = 1 << j;
    if (tid >= dd) s = fmaxf(s, a.pw[LM_CHUNK * dd] * st[cur][tid - dd]);
    cur ^= 1;
    st[cur][tid] = s;
    __syncthreads();
  }
  static_assert(LM_THREADS == 256, "8 scan rounds");
  const float prev = tid ? st[cur][tid - 1] : 0.f;  // the end state of the chunk before this one, the group starting from 0
#pragma unroll
  for (int i = 0; i < LM_CHUNK; ++i) ec[i] = fmaxf(dl[i], a.pw[i + 1] * prev);
  __syncthreads();
  float* dg = a.dg + ((long long)b * a.gmax + g) * LM_GROUP;
#pragma unroll
  for (int e = 0; e < LM_CHUNK; ++e) {
    const int q = tid + LM_THREADS * e;
    dg[q] = es[(q >> 4) * LM_ROW + (q & 15)];
  }
  if (tid == LM_THREADS - 1) a.gs[(long long)b * a.gmax + g] = s;
}

// gs[b][g]: Z_g -> D_g = max(Z_g, a^LM_GROUP D_(g-1)), in place
__global__ __launch_bounds__(LM_THREADS) void limiter_carry_kernel(const LimiterArgs a) {
  __shared__ float zs[LM_MAX_GROUPS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = a.samples[b];
  const int G = N ? (N + a.la + LM_GROUP - 1) / LM_GROUP : 0;  // <= gmax <= LM_MAX_GROUPS
  float* gs = a.gs + (long long)b * a.gmax;
  for (int i = tid; i < G; i += LM_THREADS) zs[i] = gs[i];
  __syncthreads();
  if (tid == 0) {
    const float ag = a.pw[LM_GROUP];
    float d = 0.f;
    for (int g = 0; g < G; ++g) gs[g] = d = fmaxf(zs[g], ag * d);
  }
}

template <bool I16>
__global__ __launch_bounds__(LM_TILE) void limiter_apply_kernel(const LimiterArgs a) {
  __shared__ float ds[LM_DSPAN];
  __shared__ float pm[LM_TILE / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int N = a.samples[b];
  const long long n0 = (long long)blockIdx.x * LM_TILE, n = n0 + tid;
  float* const y = a.y ? a.y + (long long)b * a.y_bs : nullptr;
  short* const pcm = a.pcm ? a.pcm + (long long)b * a.pcm_bs : nullptr;
  float* const curve = a.curve ? a.curve + (long long)b * a.curve_bs : nullptr;
  if (n0 >= N) {  // wholly behind the row: zeros up to the strides (no tile entry is read there)
    if (y && n < a.y_ld) y[n] = 0.f;
    if (pcm && n < a.pcm_ld) pcm[n] = 0;
    if (curve && n < a.curve_ld) curve[n] = 0.f;
    return;
  }
  const int Np = N + a.la;
  const float* dg = a.dg + (long long)b * a.gmax * LM_GROUP;
  const float* gs = a.gs + (long long)b * a.gmax;
  // ds[i] = the depth of position n0 + i = step n0 + i - la (0 past the row's last position: lanes behind the row read those)
  for (int i = tid; i < LM_TILE + a.la; i += LM_TILE) {
    const int j = (int)n0 + i;
    float d = 0.f;
    if (j < Np) {
      d = dg[j];
      const int g = j / LM_GROUP;
      if (g) d = fmaxf(d, a.pw[j - g * LM_GROUP + 1] * gs[g - 1]);
    }
    ds[i] = d;
  }
  __syncthreads();
  const float* dr = ds + tid + a.la;
  float acc = 0.f;
  for (int j = 0; j <= a.la; ++j) acc = fmaf(a.win[j], dr[-j], acc);
  const bool live = n < N;
  const float s = live ? fmaxf(1.f - acc, 0.f) : 0.f;
  const float xg = wave_load_row<I16>(a, (long long)b * a.in_bs, (int)n, N) * a.gain[b];
  const float v = live ? fminf(fmaxf(xg * s, -a.ceiling), a.ceiling) : 0.f;
  if (y && n < a.y_ld) y[n] = v;
  if (pcm && n < a.pcm_ld) pcm[n] = wave_pcm(v);
  if (curve && n < a.curve_ld) curve[n] = s;
  const float m = block_extreme<true>(live ? s : 1.f, pm, tid);
  if (tid == 0) a.tmin[(long long)b * a.t_ld + blockIdx.x] = m;
}

}  // namespace mi355tts
