// ITU-R BS.1770-4 integrated loudness (mono) of delivered rows and gain-to-target delivery (include/mi355tts.h "loudness"):
// FIVE launches measure, a SIXTH delivers, whatever N and B are.
//
// K-weighting is two biquads in series (shelf, then high-pass), a recurrence along the row.  With the input known, what a
// sample's output still depends on is the 4-vector s = (y1[n-1], y1[n-2], y2[n-1], y2[n-2]) (y1: the shelf's output, y2: the
// high-pass's), and s enters linearly: run from a wrong s, the outputs differ from the true ones by the filter's free response
// to the difference.  So a row is cut into chunks of LD_CHUNK samples, one per thread, 256 of them per workgroup (a GROUP of
// LD_GROUP = 16 384 samples):
//   loudness_chunk_kernel   every chunk from s = 0 (its x[n-1], x[n-2] are the row's own): its end state z.  The true end state
//                           of chunk k is s_k = z_k + M s_(k-1), M = A^LD_CHUNK, A the 4 x 4 transition matrix of the free
//                           response: a Hillis-Steele scan over the workgroup's 256 chunks (8 rounds, round j adds
//                           M^(2^j) s_(k - 2^j)) gives every chunk's end state for a group that itself starts from 0.  Also
//                           max |x| of the group.
//   loudness_carry_kernel   one workgroup per row: the groups' end states from LDS, S_g = Z_g + M^256 S_(g-1), in sequence (a
//                           row has at most 1024 groups).
//   loudness_weight_kernel  every chunk again, now from its true start state (the scan's s_(k-1) + M^k S_(g-1)): the K-weighted
//                           samples, rounded to f32, through LDS into the row.
//   loudness_segment_kernel one workgroup per hop-sized segment: the sum of squares (f64, of the f32 samples) of its first
//                           block mod hop samples and of all of them.  Thread t adds samples t, t + 256, ... in order, then a
//                           fixed tree.
//   loudness_gate_kernel    one workgroup per row: block j = segments j .. j + block div hop - 1 and the head of the next, added
//                           in that order; z_j = f32(sum / block); both gates, the integrated value, the gain.
//   loudness_apply_kernel   out = x * g, and / or its saturating int16, zeros up to the row stride.
// The matrices M^0 .. M^256 are computed on the host in double at load time and passed as data (LoudnessArgs::pw).
// The recurrence runs in f64: the weighted samples then are the f32 roundings of the float64 definition (1.5e-8 off on a 0.3
// peak, where a float32 recurrence at the high-pass's poles, radius 0.989, is 1e-5 off: profiles/loudness.md), the carried
// states add no error of their own, and the launches sit near the launch floor either way.  No sum uses an atomic, and every
// order of summation is fixed by the row alone: not by the grid, not by B.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_io.h"

namespace mi355tts {

constexpr int LD_CHUNK = 64;                    // samples per thread
constexpr int LD_THREADS = 256;                 // chunks per workgroup
constexpr int LD_GROUP = LD_CHUNK * LD_THREADS; // samples per workgroup
constexpr int LD_ROW = LD_CHUNK + 1;            // a chunk's stride in LDS: lane t walks bank t + i, no conflict
constexpr int LD_MAX_GROUPS = 1024;             // 2^24 / LD_GROUP

struct LoudnessArgs {
  const float* in_f32;  // exactly one of the two (a template parameter says which), [B][in_bs]
  const short* in_i16;
  long long in_bs;
  const int* samples;   // [B]
  double sb[3], sa[2], hb[3], ha[2];  // the ten coefficients (the caller's floats, widened)
  const double* pw;     // [257][16]: M^k row-major, M = A^LD_CHUNK
  int block, hop;
  double abs_thr;       // 10^((-70 + 0.691) / 10): the absolute gate on z
  double* cstate;       // [B][gmax * 256][4]: end state of every chunk of a group that starts from 0
  double* gstate;       // [B][gmax][4]: the same for the group's last chunk (Z_g), then its TRUE end state (S_g)
  float* gpeak;         // [B][gmax]: max |x| of the group
  int gmax;
  float* w;             // [B][w_bs]: the K-weighted row, N samples | zeros up to w_ld
  long long w_bs, w_ld;
  double* seg;          // [B][smax][2]: head and whole sum of squares per segment
  long long smax;
  float* z;             // [B][zmax]: the block mean squares
  long long zmax;
  float target, ceiling;  // target LUFS (NaN: measure only), the sample-peak ceiling
  double max_gain;        // the largest linear gain, 10^(max_gain_db / 20)
  float* res;           // [B][3]: lufs, gain, max |x|
};

// xs[t * LD_ROW + i] = x[g0 + t * 64 + i] (zeros outside the row), hx = x[g0 - 2], x[g0 - 1]: 64 coalesced loads per lane
template <bool I16>
__device__ __forceinline__ void loudness_stage(const LoudnessArgs& a, float* xs, float* hx, long long row, long long g0, int N, int tid) {
  for (int e = 0; e < LD_CHUNK; ++e) {
    const int i = e * LD_THREADS + tid;
    xs[(i >> 6) * LD_ROW + (i & 63)] = wave_load_row<I16>(a, row, g0 + i, N);
  }
  if (tid < 2) hx[tid] = wave_load_row<I16>(a, row, g0 - 2 + tid, N);
}

// one chunk of the cascade from state s (in place); x1, x2 = x[n-1], x[n-2] before it.  WRITE: the f32 outputs replace the inputs
template <bool WRITE>
__device__ __forceinline__ void loudness_run(const LoudnessArgs& a, float* xc, double x1, double x2, double s[4]) {
  double u1 = s[0], u2 = s[1], v1 = s[2], v2 = s[3];
  for (int i = 0; i < LD_CHUNK; ++i) {
    const double x0 = (double)xc[i];
    const double u0 = a.sb[0] * x0 + a.sb[1] * x1 + a.sb[2] * x2 - a.sa[0] * u1 - a.sa[1] * u2;
    const double v0 = a.hb[0] * u0 + a.hb[1] * u1 + a.hb[2] * u2 - a.ha[0] * v1 - a.ha[1] * v2;
    x2 = x1; x1 = x0;
    u2 = u1; u1 = u0;
    v2 = v1; v1 = v0;
    if constexpr (WRITE) xc[i] = (float)v0;
  }
  s[0] = u1; s[1] = u2; s[2] = v1; s[3] = v2;
}

// r += m (4 x 4, row-major) * v
__device__ __forceinline__ void loudness_madd(double r[4], const double* m, const double v[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] += m[4 * i] * v[0] + m[4 * i + 1] * v[1] + m[4 * i + 2] * v[2] + m[4 * i + 3] * v[3];
}

template <bool I16>
__global__ __launch_bounds__(LD_THREADS) void loudness_chunk_kernel(const LoudnessArgs a) {
  __shared__ float xs[LD_THREADS * LD_ROW];
  __shared__ float hx[2];
  __shared__ double st[2][LD_THREADS][4];
  __shared__ float pm[LD_THREADS / 64];
  const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const int N = a.samples[b];
  const long long g0 = (long long)g * LD_GROUP;
  if (g0 >= N) return;  // (the whole workgroup: nothing reads this group's entries)
  loudness_stage<I16>(a, xs, hx, (long long)b * a.in_bs, g0, N, tid);
  __syncthreads();
  float* xc = xs + tid * LD_ROW;
  double s[4] = {0, 0, 0, 0};
  loudness_run<false>(a, xc, tid ? (double)xc[-2] : (double)hx[1], tid ? (double)xc[-3] : (double)hx[0], s);
  float m = 0.f;
  for (int i = 0; i < LD_CHUNK; ++i) m = fmaxf(m, fabsf(xc[i]));
  m = wave_max(m);
  if ((tid & 63) == 0) pm[tid >> 6] = m;  // (read behind the scan's barriers)
  int cur = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) st[0][tid][i] = s[i];
  __syncthreads();
  for (int j = 0; j < 8; ++j) {  // after round j: s_k = sum over the last 2^(j+1) chunks i <= k of M^(k - i) z_i
    const int d = 1 << j;
    if (tid >= d) {
      double v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = st[cur][tid - d][i];
      loudness_madd(s, a.pw + 16 * d, v);
    }
    cur ^= 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) st[cur][tid][i] = s[i];
    __syncthreads();
  }
  double* cs = a.cstate + (((long long)b * a.gmax + g) * LD_THREADS + tid) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) cs[i] = s[i];
  if (tid == LD_THREADS - 1) {
    double* gs = a.gstate + ((long long)b * a.gmax + g) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) gs[i] = s[i];
  }
  if (tid == 0) a.gpeak[(long long)b * a.gmax + g] = block_extreme_of<false>(pm);
}

// gstate[b][g]: Z_g -> S_g = Z_g + M^256 S_(g-1), in place
__global__ __launch_bounds__(LD_THREADS) void loudness_carry_kernel(const LoudnessArgs a) {
  __shared__ double zs[LD_MAX_GROUPS * 4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = a.samples[b];
  const int G = (int)(((long long)N + LD_GROUP - 1) / LD_GROUP);  // <= gmax <= LD_MAX_GROUPS
  double* gs = a.gstate + (long long)b * a.gmax * 4;
  for (int i = tid; i < 4 * G; i += LD_THREADS) zs[i] = gs[i];
  __syncthreads();
  if (tid == 0) {
    double s[4] = {0, 0, 0, 0};
    for (int g = 0; g < G; ++g) {
      double r[4] = {zs[4 * g], zs[4 * g + 1], zs[4 * g + 2], zs[4 * g + 3]};
      loudness_madd(r, a.pw + 16 * LD_THREADS, s);
#pragma unroll
      for (int i = 0; i < 4; ++i) gs[4 * g + i] = s[i] = r[i];
    }
  }
}

template <bool I16>
__global__ __launch_bounds__(LD_THREADS) void loudness_weight_kernel(const LoudnessArgs a) {
  __shared__ float xs[LD_THREADS * LD_ROW];
  __shared__ float hx[2];
  const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const int N = a.samples[b];
  const long long g0 = (long long)g * LD_GROUP;
  float* const w = a.w + (long long)b * a.w_bs;
  if (g0 >= N) {  // wholly behind the row: zeros up to its stride
    for (int e = 0; e < LD_CHUNK; ++e) {
      const long long n = g0 + e * LD_THREADS + tid;
      if (n < a.w_ld) w[n] = 0.f;
    }
    return;
  }
  loudness_stage<I16>(a, xs, hx, (long long)b * a.in_bs, g0, N, tid);
  __syncthreads();
  // the chunk's true start state: the scan's end state of the chunk before it, plus M^tid times the group's own start state
  double s[4] = {0, 0, 0, 0};
  if (tid) {
    const double* cs = a.cstate + (((long long)b * a.gmax + g) * LD_THREADS + tid - 1) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = cs[i];
  }
  if (g) {
    const double* gs = a.gstate + ((long long)b * a.gmax + g - 1) * 4;
    const double v[4] = {gs[0], gs[1], gs[2], gs[3]};
    loudness_madd(s, a.pw + 16 * tid, v);
  }
  float* xc = xs + tid * LD_ROW;
  const double x1 = tid ? (double)xc[-2] : (double)hx[1], x2 = tid ? (double)xc[-3] : (double)hx[0];
  __syncthreads();  // the chunk before this one is overwritten by its thread: its last two inputs are read first
  loudness_run<true>(a, xc, x1, x2, s);
  __syncthreads();
  for (int e = 0; e < LD_CHUNK; ++e) {
    const int i = e * LD_THREADS + tid;
    const long long n = g0 + i;
    if (n < a.w_ld) w[n] = n < N ? xs[(i >> 6) * LD_ROW + (i & 63)] : 0.f;
  }
}

// the fixed tree behind every per-thread partial sum: 256 -> 1, result in red[0] (all threads may read it after the call)
__device__ __forceinline__ void loudness_tree(double* red, int tid) {
  for (int d = LD_THREADS / 2; d >= 1; d >>= 1) {
    __syncthreads();
    if (tid < d) red[tid] += red[tid + d];
  }
  __syncthreads();
}

__global__ __launch_bounds__(LD_THREADS) void loudness_segment_kernel(const LoudnessArgs a) {
  __shared__ double rh[LD_THREADS], rf[LD_THREADS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long sg = blockIdx.x;
  const int N = a.samples[b];
  const long long n0 = sg * a.hop;
  if (n0 >= N) return;
  const float* w = a.w + (long long)b * a.w_bs;
  const int head = a.block % a.hop;
  const int len = (int)((long long)a.hop < N - n0 ? (long long)a.hop : N - n0);
  double h = 0, r = 0;
  for (int i = tid; i < len; i += LD_THREADS) {
    const double v = (double)w[n0 + i];
    if (i < head) h += v * v;
    else r += v * v;
  }
  rh[tid] = h;
  rf[tid] = r;
  loudness_tree(rh, tid);
  loudness_tree(rf, tid);
  if (tid == 0) {
    double* o = a.seg + ((long long)b * a.smax + sg) * 2;
    o[0] = rh[0];
    o[1] = rh[0] + rf[0];
  }
}

__global__ __launch_bounds__(LD_THREADS) void loudness_gate_kernel(const LoudnessArgs a) {
  __shared__ double red[LD_THREADS];
  __shared__ double cnt[LD_THREADS];
  __shared__ float pm[LD_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = a.samples[b];
  const long long S = ((long long)N + a.hop - 1) / a.hop;
  const long long nb = N >= a.block ? (long long)(N - a.block) / a.hop + 1 : (N > 0 ? 1 : 0);
  const int q = a.block / a.hop, head = a.block % a.hop;
  const double* seg = a.seg + (long long)b * a.smax * 2;
  float* z = a.z + (long long)b * a.zmax;
  const int G = (int)(((long long)N + LD_GROUP - 1) / LD_GROUP);
  float m = 0.f;
  for (int g = tid; g < G; g += LD_THREADS) m = fmaxf(m, a.gpeak[(long long)b * a.gmax + g]);
  pm[tid] = m;
  // the block mean squares, and the sum and count of those past the absolute gate
  double sum = 0, n = 0;
  for (long long j = tid; j < nb; j += LD_THREADS) {
    double e = 0;
    if (N < a.block) {  // the short row: ONE block of its N samples
      for (long long k = 0; k < S; ++k) e += seg[2 * k + 1];
      e /= (double)N;
    } else {
      for (int k = 0; k < q; ++k) e += seg[2 * (j + k) + 1];
      if (head) e += seg[2 * (j + q)];
      e /= (double)a.block;
    }
    const float zj = (float)e;
    z[j] = zj;
    if ((double)zj > a.abs_thr) {
      sum += (double)zj;
      n += 1;
    }
  }
  red[tid] = sum;
  cnt[tid] = n;
  loudness_tree(red, tid);
  loudness_tree(cnt, tid);
  const double n_abs = cnt[0];
  const double rel_thr = n_abs > 0 ? 0.1 * (red[0] / n_abs) : 0;  // -10 LU under the absolutely gated mean
  __syncthreads();
  sum = 0;
  n = 0;
  for (long long j = tid; j < nb; j += LD_THREADS) {
    const double zj = (double)z[j];  // (this thread's own stores)
    if (zj > a.abs_thr && zj > rel_thr) {
      sum += zj;
      n += 1;
    }
  }
  red[tid] = sum;
  cnt[tid] = n;
  loudness_tree(red, tid);
  loudness_tree(cnt, tid);
  for (int d = LD_THREADS / 2; d >= 1; d >>= 1) {
    if (tid < d) pm[tid] = fmaxf(pm[tid], pm[tid + d]);
    __syncthreads();
  }
  if (tid == 0) {
    const float peak = pm[0];
    const float lufs = cnt[0] > 0 ? (float)(-0.691 + 10.0 * log10(red[0] / cnt[0])) : -INFINITY;
    double gain = 1.0;
    if (a.target == a.target && cnt[0] > 0) {  // a target, and something to measure
      gain = pow(10.0, ((double)a.target - (double)lufs) / 20.0);
      gain = gain < a.max_gain ? gain : a.max_gain;
      if (peak > 0.f) {
        const double cap = (double)a.ceiling / (double)peak;
        gain = gain < cap ? gain : cap;
      }
    }
    float gf = (float)gain;
    // the rounding of g may carry the largest sample one ulp past the ceiling: g steps down until it does not (once, at most twice)
    if (a.target == a.target && cnt[0] > 0 && peak > 0.f)
      for (int i = 0; i < 4 && peak * gf > a.ceiling; ++i) gf = __uint_as_float(__float_as_uint(gf) - 1);
    float* r = a.res + 3 * b;
    r[0] = lufs;
    r[1] = gf;
    r[2] = peak;
  }
}

// out rows [B][o_bs]: N samples of x * g | zeros up to o_ld
template <bool I16>
__global__ __launch_bounds__(256) void loudness_apply_kernel(const LoudnessArgs a, float* out_f32, short* out_i16, long long o_bs, long long o_ld) {
  const int b = blockIdx.y;
  const int N = a.samples[b];
  const float g = a.res[3 * b + 1];
  const long long row = (long long)b * a.in_bs;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < o_ld; i += step) {
    const float y = i < N ? wave_load_row<I16>(a, row, i, N) * g : 0.f;
    if (out_f32) out_f32[(long long)b * o_bs + i] = y;
    if (out_i16) out_i16[(long long)b * o_bs + i] = wave_pcm(y);
  }
}

}  // namespace mi355tts
