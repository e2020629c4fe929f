// Griffin-Lim vocoder: mel -> waveform with no weights (larynx/griffin_lim.py:22-76 on the STFT helpers of
// larynx/audio.py:232-306).  The reference's conventions, kept exactly: 1024-point frames every 256 samples, symmetric
// np.hanning(1024) on analysis AND synthesis, no window-sum normalisation, frames at range(0, len - 1024, 256); the
// magnitudes are exp(mel) @ mel_basis * mel_scaling with the LAST mel frame dropped (griffin_lim.py:57), so a mel of F frames
// gives T = F - 1 STFT frames and a signal of T * 256 + 1024 samples.
//
//   griffin_lim_mag_kernel   mag[b][t][k] = scale * sum_m exp(mel[b][m][t]) * basis[m][k]          (once per call)
//   griffin_lim_init_kernel  frame t of inverse(mag, phase0): phase injected or drawn on the device  (once per call)
//   griffin_lim_iter_kernel  ONE Griffin-Lim iteration (transform + inverse) of one frame            (once per iteration)
//   griffin_lim_out_kernel   overlap-add of the last frame buffer into the waveform + the row's peak (once per call)
//   griffin_lim_int16_kernel audio_float_to_int16 (larynx/audio.py:118-125)                          (once per call, optional)
//
// The iteration kernel (the hot path): one workgroup = ONE WAVE = one frame.  Its 1024 input samples are the sum of the up to
// 7 synthesis frames of the previous iteration that overlap it, read from a ping-pong frame buffer in frame order (the
// reference's `x[i : i + 1024] += ...` order): overlap-add on read, so there is no waveform between two iterations.
//
// FFT layout.  The real 1024-point transform is a 512-point complex one (z[j] = x[2j] + i x[2j+1]) plus a pair-wise
// post-pass; the 512-point transform is three radix-8 Stockham passes (Ns = 1, 8, 64), each lane holding its 8 points in
// registers, so a transform has 2 LDS exchanges inside (not ten radix-2 stages) and needs no bit reversal.  The first pass
// takes its points straight from the gather registers (lane j owns samples 2j + 128r, 2j + 128r + 1: one coalesced 8-byte load
// per lane), the last pass of the inverse transform leaves the output samples in registers in that same ownership.  LDS holds
// float2 values at index a + (a >> 3): with 8-byte accesses every store of the three passes and of the pair pass is
// conflict-free and the stride-1 loads meet a 2-way conflict on 3 of 32 lanes.  Lane j then owns the bin pairs (k, 512 - k),
// k = j + 64q: it unpacks X[k] and X[512 - k] from Z[k], Z[512 - k], replaces their magnitudes, packs the two bins of the
// inverse transform's input and stores them where it read — forward and inverse transform share one exchange.
//
// The angle is never formed: the reference computes angle = arctan2(im, re) and then mag * cos(angle), mag * sin(angle);
// cos(atan2(im, re)) = re / |S| and sin(atan2(im, re)) = im / |S|, so the new spectrum is mag * S / |S| — no transcendental
// in the loop, and one rounding less than going through the angle.  |S| = 0 gives (mag, 0), as arctan2(0, 0) = 0 does.
// |S| is formed from S / max(|re|, |im|): nothing unscaled is squared.  The kernels are f32 throughout: an input whose
// signal or spectrum leaves the f32 range (a mel that is not in the ln domain: magnitudes beyond ~1e30) is out of scope.
//
// Window and twiddles come from a table the context builds once in double precision (gl_build_table): tab[0 .. 1023] the
// window, then 1024 float2 e^{-2 pi i m / 1024}.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "small_kernels.h"

namespace mi355tts {

constexpr int GL_FFT = 1024;
constexpr int GL_HOP = 256;
constexpr int GL_BINS = GL_FFT / 2 + 1;
constexpr int GL_HALF = GL_FFT / 2;          // points of the complex transform
constexpr int GL_MAG_LD = 516;               // row stride of mag[b][t][:]
constexpr int GL_LDS = GL_HALF + GL_HALF / 8;  // padded float2 slots
constexpr int GL_TAB_FLOATS = GL_FFT + 2 * GL_FFT;
constexpr int GL_MAX_MELS = 256;
constexpr int GL_MAG_FRAMES = 8;  // frames per workgroup of the magnitude kernel

__device__ __forceinline__ int gl_pad(int a) { return a + (a >> 3); }
__device__ __forceinline__ float2 gl_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// 8-point DFT (forward sign), natural order in and out
__device__ __forceinline__ void gl_dft8(float2 (&v)[8]) {
  constexpr float H = 0.70710678118654752f;
  float2 s[4], d[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s[i] = make_float2(v[i].x + v[i + 4].x, v[i].y + v[i + 4].y);
    d[i] = make_float2(v[i].x - v[i + 4].x, v[i].y - v[i + 4].y);
  }
  d[1] = make_float2((d[1].x + d[1].y) * H, (d[1].y - d[1].x) * H);   // * (1 - i) / sqrt 2
  d[2] = make_float2(d[2].y, -d[2].x);                                // * -i
  d[3] = make_float2((d[3].y - d[3].x) * H, -(d[3].x + d[3].y) * H);  // * (-1 - i) / sqrt 2
  auto dft4 = [](const float2(&x)[4], float2& y0, float2& y1, float2& y2, float2& y3) {
    const float2 t0 = make_float2(x[0].x + x[2].x, x[0].y + x[2].y), t1 = make_float2(x[0].x - x[2].x, x[0].y - x[2].y);
    const float2 t2 = make_float2(x[1].x + x[3].x, x[1].y + x[3].y);
    const float2 t3 = make_float2(x[1].y - x[3].y, -(x[1].x - x[3].x));  // (x1 - x3) * -i
    y0 = make_float2(t0.x + t2.x, t0.y + t2.y);
    y2 = make_float2(t0.x - t2.x, t0.y - t2.y);
    y1 = make_float2(t1.x + t3.x, t1.y + t3.y);
    y3 = make_float2(t1.x - t3.x, t1.y - t3.y);
  };
  dft4(s, v[0], v[2], v[4], v[6]);
  dft4(d, v[1], v[3], v[5], v[7]);
}

// 512-point forward transform.  In: v[r] = z[j + 64 r].  Out: Z[j + 64 r] in v[r], and (STORE) at p[gl_pad(j + 64 r)].  `p` may
// still be read by other lanes when the call starts; `q` must not be.
template <bool STORE>
__device__ __forceinline__ void gl_fft512(float2 (&v)[8], float2* p, float2* q, const float2* __restrict__ tw, int j) {
  gl_dft8(v);  // Ns = 1: no twiddles
#pragma unroll
  for (int r = 0; r < 8; ++r) q[gl_pad(8 * j + r)] = v[r];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = q[gl_pad(j + 64 * r)];
  {
    const int k = j & 7;  // Ns = 8: e^{-2 pi i r k / 64}
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = gl_cmul(v[r], tw[16 * r * k]);
  }
  gl_dft8(v);
  {
    const int base = (j >> 3) * 64 + (j & 7);
#pragma unroll
    for (int r = 0; r < 8; ++r) p[gl_pad(base + 8 * r)] = v[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = p[gl_pad(j + 64 * r)];
#pragma unroll
  for (int r = 1; r < 8; ++r) v[r] = gl_cmul(v[r], tw[2 * r * j]);  // Ns = 64: e^{-2 pi i r j / 512}
  gl_dft8(v);
  if (STORE) {
#pragma unroll
    for (int r = 0; r < 8; ++r) q[gl_pad(j + 64 * r)] = v[r];
    __syncthreads();
  }
}

// g * S / |S|; S = 0 -> (g, 0)
__device__ __forceinline__ float2 gl_rephase(float2 s, float g) {
  const float m = fmaxf(fabsf(s.x), fabsf(s.y));
  if (!(m > 0.f)) return make_float2(g, 0.f);
  const float rx = s.x / m, ry = s.y / m;
  const float sc = g / sqrtf(rx * rx + ry * ry);
  return make_float2(rx * sc, ry * sc);
}

// The packed input of the inverse transform for the bin pair (k, 512 - k), 0 < k < 256, from the spectrum values yk = Y[k],
// yn = Y[512 - k] (w = e^{-2 pi i k / 1024}); stored conjugated: IFFT(Z) = conj(FFT(conj Z)) / N.
__device__ __forceinline__ void gl_pack_pair(float2* a, int k, float2 yk, float2 yn, float2 w) {
  const float2 e = make_float2(0.5f * (yk.x + yn.x), 0.5f * (yk.y - yn.y));
  const float2 o = gl_cmul(make_float2(0.5f * (yk.x - yn.x), 0.5f * (yk.y + yn.y)), make_float2(w.x, -w.y));
  a[gl_pad(k)] = make_float2(e.x - o.y, -(e.y + o.x));            // conj(E + i O)
  a[gl_pad(GL_HALF - k)] = make_float2(e.x + o.y, -(o.x - e.y));  // conj(conj E + i conj O)
}
// bins 0 and 512 (real: irfft ignores their imaginary parts) and bin 256
__device__ __forceinline__ void gl_pack_dc(float2* a, float y0, float y512) { a[0] = make_float2(0.5f * (y0 + y512), -0.5f * (y0 - y512)); }
__device__ __forceinline__ void gl_pack_mid(float2* a, float2 y256) { a[gl_pad(GL_HALF / 2)] = y256; }  // conj(conj Y)

// inverse transform of the packed spectrum in `a`, synthesis window, frame store.  Every lane of the wave must arrive.
__device__ __forceinline__ void gl_synthesize(float2* a, float2* bq, const float* __restrict__ tab, int j, float* __restrict__ frame) {
  const float2* tw = reinterpret_cast<const float2*>(tab + GL_FFT);
  const float2* win = reinterpret_cast<const float2*>(tab);
  __syncthreads();
  float2 v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = a[gl_pad(j + 64 * r)];
  gl_fft512<false>(v, a, bq, tw, j);
  float2* out = reinterpret_cast<float2*>(frame);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const float2 w = win[j + 64 * r];
    out[j + 64 * r] = make_float2(w.x * (v[r].x * (1.0f / GL_HALF)), w.y * (-v[r].y * (1.0f / GL_HALF)));
  }
}

// uniform phase of (seed, row, bin, frame): u = a 24-bit uniform in [0, 1) from the counter hash of the noise generator
// (pcg_hash, small_kernels.h), phase = np.angle(np.exp(2j pi u)) = 2 pi u for u <= 1/2, 2 pi (u - 1) above.  The factor is the
// f32 just BELOW 2 pi, so the phase lies strictly inside (-pi, pi) as an exact real number.
__device__ __forceinline__ float gl_draw_phase(uint64_t seed, uint32_t k, uint32_t t) {
  const uint32_t key = pcg_hash((uint32_t)seed ^ pcg_hash((uint32_t)(seed >> 32) + 0x9e3779b9u));
  const uint32_t x = pcg_hash(key ^ pcg_hash(0x51ed270bu + k) ^ (t * 0xc2b2ae35u));
  const float u = (float)(x >> 8) * (1.0f / 16777216.0f);
  return 6.2831850f * (u > 0.5f ? u - 1.0f : u);
}

// mag[b][t][k] = scale * sum_m exp(mel[b][m][t]) * basis[m][k], t < frames[b] - 1.  8 frames per workgroup: the basis is read
// once per 8 frames, coalesced along k; sum in m order.
__global__ __launch_bounds__(256) void griffin_lim_mag_kernel(const float* __restrict__ mel, long long mel_bs, int mel_ld,
                                                              const int* __restrict__ frames, int M, const float* __restrict__ basis,
                                                              float scale, float* __restrict__ mag, int Tmax) {
  __shared__ float e[GL_MAX_MELS * GL_MAG_FRAMES];
  const int b = blockIdx.y, t0 = blockIdx.x * GL_MAG_FRAMES, tid = threadIdx.x;
  const int T = frames[b] - 1;
  if (t0 >= T) return;
  for (int i = tid; i < M * GL_MAG_FRAMES; i += 256) {
    const int m = i / GL_MAG_FRAMES, t = t0 + i % GL_MAG_FRAMES;
    e[i] = t < T ? expf(mel[(long long)b * mel_bs + (long long)m * mel_ld + t]) : 0.f;
  }
  __syncthreads();
  for (int k = tid; k < GL_BINS; k += 256) {
    float acc[GL_MAG_FRAMES];
#pragma unroll
    for (int u = 0; u < GL_MAG_FRAMES; ++u) acc[u] = 0.f;
    for (int m = 0; m < M; ++m) {
      const float w = basis[m * GL_BINS + k];
#pragma unroll
      for (int u = 0; u < GL_MAG_FRAMES; ++u) acc[u] = fmaf(e[m * GL_MAG_FRAMES + u], w, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < GL_MAG_FRAMES; ++u)
      if (t0 + u < T) mag[((long long)b * Tmax + t0 + u) * GL_MAG_LD + k] = acc[u] * scale;
  }
}

// frame n of inverse(mag, phase) (larynx/audio.py:272-289): Y[k] = mag[k] (cos phase, sin phase).  phase0 [B][513][ph_ld]
// injected, or nullptr: drawn (row b from the stream seed + b).  phase_out (optional, same layout) receives the phase used.
__global__ __launch_bounds__(64) void griffin_lim_init_kernel(const float* __restrict__ mag, const int* __restrict__ frames, int Tmax,
                                                              const float* __restrict__ phase0, float* __restrict__ phase_out, int ph_ld,
                                                              uint64_t seed, const float* __restrict__ tab, float* __restrict__ fout) {
  __shared__ float2 a[GL_LDS], bq[GL_LDS];
  const int b = blockIdx.y, n = blockIdx.x, j = threadIdx.x;
  if (n >= frames[b] - 1) return;
  const float2* tw = reinterpret_cast<const float2*>(tab + GL_FFT);
  const float* mg = mag + ((long long)b * Tmax + n) * GL_MAG_LD;
  const long long pb = (long long)b * GL_BINS * ph_ld + n;
  auto spec = [&](int k) {
    const float ph = phase0 ? phase0[pb + (long long)k * ph_ld] : gl_draw_phase(seed + (uint64_t)b, (uint32_t)k, (uint32_t)n);
    if (phase_out) phase_out[pb + (long long)k * ph_ld] = ph;
    const float g = mg[k];
    return make_float2(g * cosf(ph), g * sinf(ph));
  };
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = j + 64 * q;
    const float2 yk = spec(k), yn = spec(GL_HALF - k);
    if (k == 0) gl_pack_dc(a, yk.x, yn.x);
    else gl_pack_pair(a, k, yk, yn, tw[k]);
  }
  if (j == 0) gl_pack_mid(a, spec(GL_HALF / 2));
  gl_synthesize(a, bq, tab, j, fout + ((long long)b * Tmax + n) * GL_FFT);
}

// One Griffin-Lim iteration of frame n: `_, angles = transform(signal); signal = inverse(magnitudes, angles)`
// (larynx/griffin_lim.py:72-74) with the signal kept as its synthesis frames (fin -> fout, [B][Tmax][1024]).
__global__ __launch_bounds__(64) void griffin_lim_iter_kernel(const float* __restrict__ fin, float* __restrict__ fout,
                                                              const float* __restrict__ mag, const int* __restrict__ frames, int Tmax,
                                                              const float* __restrict__ tab) {
  __shared__ float2 a[GL_LDS], bq[GL_LDS];
  const int b = blockIdx.y, n = blockIdx.x, j = threadIdx.x;
  const int T = frames[b] - 1;
  if (n >= T) return;
  const float2* tw = reinterpret_cast<const float2*>(tab + GL_FFT);
  const float2* win = reinterpret_cast<const float2*>(tab);
  // the frame's samples 2j + 128r (+ 1) of the overlap-added signal: frame m = n - d contributes its samples at + 256 d, in
  // frame order; r + 2d in [0, 8) decides (for the whole wave) whether frame m covers the pair
  float2 v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = make_float2(0.f, 0.f);
#pragma unroll
  for (int d = 3; d >= -3; --d) {
    const int m = n - d;
    if (m < 0 || m >= T) continue;
    const float2* src = reinterpret_cast<const float2*>(fin + ((long long)b * Tmax + m) * GL_FFT + 256 * d);
#pragma unroll
    for (int r = 0; r < 8; ++r)
      if (r + 2 * d >= 0 && r + 2 * d < 8) {
        const float2 x = src[j + 64 * r];
        v[r].x += x.x;
        v[r].y += x.y;
      }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const float2 w = win[j + 64 * r];
    v[r].x *= w.x;
    v[r].y *= w.y;
  }
  gl_fft512<true>(v, bq, a, tw, j);  // Z in a
  const float* mg = mag + ((long long)b * Tmax + n) * GL_MAG_LD;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = j + 64 * q;
    const float2 zk = a[gl_pad(k)];
    if (k == 0) {
      // X[0] = Re Z0 + Im Z0, X[512] = Re Z0 - Im Z0: real, so the new bins are +-mag (arctan2(0, x) is 0 or pi)
      const float x0 = zk.x + zk.y, x512 = zk.x - zk.y;
      gl_pack_dc(a, x0 < 0.f ? -mg[0] : mg[0], x512 < 0.f ? -mg[GL_HALF] : mg[GL_HALF]);
    } else {
      const float2 zn = a[gl_pad(GL_HALF - k)];
      const float2 w = tw[k];
      const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
      const float2 o = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));  // -i / 2 (Z[k] - conj Z[512 - k])
      const float2 wo = gl_cmul(w, o);
      const float2 xk = make_float2(e.x + wo.x, e.y + wo.y);     // X[k]
      const float2 xn = make_float2(e.x - wo.x, -(e.y - wo.y));  // X[512 - k]
      gl_pack_pair(a, k, gl_rephase(xk, mg[k]), gl_rephase(xn, mg[GL_HALF - k]), w);
    }
  }
  if (j == 0) {
    const float2 z = a[gl_pad(GL_HALF / 2)];
    gl_pack_mid(a, gl_rephase(make_float2(z.x, -z.y), mg[GL_HALF / 2]));  // X[256] = conj Z[256]
  }
  gl_synthesize(a, bq, tab, j, fout + ((long long)b * Tmax + n) * GL_FFT);
}

// wav[b][s] = sum over the (up to 4) frames covering sample s, in frame order; length (frames[b] - 1) * 256 + 1024, zeros up
// to ld; peak_bits[b] (optional) = max |wav[b][:]| as uint bits.
__global__ __launch_bounds__(256) void griffin_lim_out_kernel(const float* __restrict__ fb, int Tmax, const int* __restrict__ frames,
                                                              float* __restrict__ wav, long long bs, long long ld, unsigned* peak_bits) {
  __shared__ float red[4];
  const int b = blockIdx.y;
  const int T = frames[b] - 1;
  const long long len = T > 0 ? (long long)T * GL_HOP + GL_FFT : 0;
  float mx = 0.f;
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < ld; s += (long long)gridDim.x * 256) {
    float acc = 0.f;
    if (s < len) {
      const int n0 = s < GL_FFT ? 0 : (int)((s - (GL_FFT - GL_HOP)) / GL_HOP);
      int n1 = (int)(s / GL_HOP);
      if (n1 > T - 1) n1 = T - 1;
      for (int n = n0; n <= n1; ++n) acc += fb[((long long)b * Tmax + n) * GL_FFT + (s - (long long)n * GL_HOP)];
    }
    wav[(long long)b * bs + s] = acc;
    mx = fmaxf(mx, fabsf(acc));
  }
  if (!peak_bits) return;
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(&peak_bits[b], __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// audio_float_to_int16 (larynx/audio.py:118-125): a * 32767 / max(0.01, peak), clip, truncate toward zero; zeros past the row
__global__ __launch_bounds__(256) void griffin_lim_int16_kernel(const float* __restrict__ wav, long long bs, const int* __restrict__ frames,
                                                                const unsigned* __restrict__ peak_bits, short* __restrict__ out,
                                                                long long out_bs, long long out_ld) {
  const int b = blockIdx.y;
  const int T = frames[b] - 1;
  const long long len = T > 0 ? (long long)T * GL_HOP + GL_FFT : 0;
  const float g = 32767.0f / fmaxf(0.01f, __uint_as_float(peak_bits[b]));
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < out_ld; s += (long long)gridDim.x * 256) {
    short r = 0;
    if (s < len) r = (short)(int)fminf(fmaxf(wav[(long long)b * bs + s] * g, -32767.0f), 32767.0f);
    out[(long long)b * out_bs + s] = r;
  }
}

}  // namespace mi355tts
