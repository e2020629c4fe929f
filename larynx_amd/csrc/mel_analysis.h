// Mel analysis: waveform -> the two planes of a mi355tts_mel, ONE launch per call (the inverse direction of griffin_lim.h and of
// mel_transform, small_kernels.h).  1024-point frames every 256 samples, magnitudes, the mel filter bank, then the voice's own
// domain: the vocoder plane (ln of the clamped amplitude: dynamic_range_compression, larynx/audio.py:106-108) and the raw plane
// (amp_to_db + AudioSettings.normalize, audio.py:55-81 — the inverse of mel_transform, switch by switch).
//
// Two framings, which differ only in the index map, the window table and the frame count:
//   MI355TTS_FRAMING_HIFIGAN    the published HiFi-GAN training convention — NOT a line of the reference, which has no analysis
//                               on its inference path: reflect-pad 384 samples each side, so frame t reads 256 t - 384 + i (an
//                               index < 0 -> -idx, >= N -> 2 (N - 1) - idx), periodic Hann; F = N / 256 frames, N >= 385 (one
//                               reflection must be enough), frame t centred on hop t
//   MI355TTS_FRAMING_REFERENCE  the reference's own stft (larynx/audio.py:232-249): no padding, frame t reads x[256 t : 256 t +
//                               1024), symmetric np.hanning(1024); T = ceil((N - 1024) / 256) frames for N > 1024
//
// One WAVE per frame, as in griffin_lim_iter_kernel, MA_FRAMES frames of one row per workgroup.  A wave gathers its 1024 samples
// in the ownership gl_fft512 expects (lane j: samples 2j + 128 r, 2j + 128 r + 1; float or int16 source, s * 2^-15 is exact),
// windows them, runs the 512-point complex transform and the pair-wise unpack of griffin_lim.h to bins 0 .. 512 and leaves
// mag[k] = sqrt(re^2 + im^2 + mag_eps) in its LDS slice (|x| <= 1 gives |X| <= 1024: nothing to rescale before the square).
// Lane l then sums channels l, l + 64, .. over the channel's non-zero band [k0, k1) of the basis only (the Slaney triangles hold
// ~2 x 513 non-zeros against 80 x 513 dense; the band table is made from the uploaded basis, so any basis works), k ascending,
// one fma per term.  The planes are [B][M][ld] with time fastest: the workgroup stages its frames' values in LDS and writes
// every channel as ONE 16-byte store per plane instead of MA_FRAMES stores `ld` floats apart.  The barriers are
// __syncthreads(): the waves of a workgroup past the row's frame count stay in every barrier (they transform zeros and
// contribute the zeros of the tail); a workgroup WHOLLY past the row writes the tail's zeros and leaves together.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "griffin_lim.h"

namespace mi355tts {

constexpr int MA_FRAMES = 4;  // frames (waves) per workgroup = floats per store: ld is a multiple of 4
constexpr int MA_PAD = (GL_FFT - GL_HOP) / 2;  // 384: the HiFi-GAN framing's reflection

struct MelAnalysisArgs {
  const float* wav_f32;   // exactly one of the two
  const short* wav_i16;
  long long wav_bs;       // samples between rows
  const int* samples;     // [B]
  const int* frames;      // [B]
  const float* window;    // [1024]: the framing's
  const float2* tw;       // [1024]: e^{-2 pi i m / 1024}
  const float* basis;     // [M][513]
  const int2* band;       // [M]: first non-zero bin, one past the last
  float* raw;
  float* voc;             // [B][M][ld]
  int M, ld, reflect;
  float mag_eps;
  MelTransform mt;
  int plain;              // no audio settings: both planes ln(max(amp, 1e-5))
};

// AudioSettings.normalize (larynx/audio.py:65-81) in its operation order
__device__ __forceinline__ float mel_normalize(float v, const MelTransform& m) {
  float n = ((v - m.ref_level_db) - m.min_level_db) / (-m.min_level_db);
  if (m.symmetric_norm) {
    n = ((2.0f * m.max_norm) * n) - m.max_norm;
    if (m.clip_norm) n = fminf(fmaxf(n, -m.max_norm), m.max_norm);
  } else {
    n = m.max_norm * n;
    if (m.clip_norm) n = fminf(fmaxf(n, 0.f), m.max_norm);
  }
  return n;
}

__global__ __launch_bounds__(64 * MA_FRAMES) void mel_analysis_kernel(MelAnalysisArgs A) {
  __shared__ float2 lds[MA_FRAMES][2][GL_LDS];
  __shared__ __attribute__((aligned(16))) float stage[2][GL_MAX_MELS][MA_FRAMES];
  const int b = blockIdx.y, t0 = blockIdx.x * MA_FRAMES, tid = threadIdx.x;
  const int wave = tid >> 6, j = tid & 63;
  const int F = A.frames[b];
  const long long plane_b = (long long)b * A.M * A.ld + t0;
  // channel m of plane p (0 raw, 1 vocoder), frames t0 .. t0 + 3: 16-byte aligned (ld and t0 are multiples of 4)
  auto run = [&](int i) {
    const bool p = i >= A.M;
    return reinterpret_cast<float4*>((p ? A.voc : A.raw) + plane_b + (long long)(p ? i - A.M : i) * A.ld);
  };
  if (t0 >= F) {  // the row's tail: zeros (the whole workgroup leaves together)
    for (int i = tid; i < 2 * A.M; i += 64 * MA_FRAMES) *run(i) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const int t = t0 + wave;
  const bool live = t < F;
  float2* a = lds[wave][0];
  float2* bq = lds[wave][1];
  float2 v[8];
  if (live) {
    const int N = A.samples[b];
    const long long row = (long long)b * A.wav_bs;
    const int base = GL_HOP * t - (A.reflect ? MA_PAD : 0);
    auto sample = [&](int i) {
      int idx = base + i;
      if (A.reflect) idx = idx < 0 ? -idx : idx >= N ? 2 * (N - 1) - idx : idx;
      return A.wav_f32 ? A.wav_f32[row + idx] : (float)A.wav_i16[row + idx] * (1.0f / 32768);
    };
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = 2 * j + 128 * r;
      v[r] = make_float2(sample(i) * A.window[i], sample(i + 1) * A.window[i + 1]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = make_float2(0.f, 0.f);
  }
  gl_fft512<true>(v, bq, a, A.tw, j);  // Z in a
  float* mag = reinterpret_cast<float*>(bq);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = j + 64 * q;
    const float2 zk = a[gl_pad(k)];
    if (k == 0) {
      const float x0 = zk.x + zk.y, x512 = zk.x - zk.y;  // real
      mag[0] = sqrtf(x0 * x0 + A.mag_eps);
      mag[GL_HALF] = sqrtf(x512 * x512 + A.mag_eps);
    } else {
      const float2 zn = a[gl_pad(GL_HALF - k)];
      const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
      const float2 o = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));  // -i / 2 (Z[k] - conj Z[512 - k])
      const float2 wo = gl_cmul(A.tw[k], o);
      const float2 xk = make_float2(e.x + wo.x, e.y + wo.y);  // X[k]
      const float2 xn = make_float2(e.x - wo.x, e.y - wo.y);  // conj X[512 - k]
      mag[k] = sqrtf(xk.x * xk.x + xk.y * xk.y + A.mag_eps);
      mag[GL_HALF - k] = sqrtf(xn.x * xn.x + xn.y * xn.y + A.mag_eps);
    }
  }
  if (j == 0) {
    const float2 z = a[gl_pad(GL_HALF / 2)];  // X[256] = conj Z[256]
    mag[GL_HALF / 2] = sqrtf(z.x * z.x + z.y * z.y + A.mag_eps);
  }
  __syncthreads();
  for (int m = j; m < A.M; m += 64) {
    float r = 0.f, u = 0.f;
    if (live) {
      const int2 kk = A.band[m];
      const float* bm = A.basis + (long long)m * GL_BINS;
      float amp = 0.f;
      for (int k = kk.x; k < kk.y; ++k) amp = fmaf(bm[k], mag[k], amp);
      const float ln = logf(fmaxf(amp, 1e-5f));
      if (A.plain) {
        r = u = ln;
      } else {
        u = A.mt.do_drc ? ln : amp;
        r = A.mt.convert_db_to_amp ? A.mt.spec_gain * log10f(fmaxf(1e-5f, amp)) : u;
        if (A.mt.signal_norm) r = mel_normalize(r, A.mt);
      }
    }
    stage[0][m][wave] = r;
    stage[1][m][wave] = u;
  }
  __syncthreads();
  for (int i = tid; i < 2 * A.M; i += 64 * MA_FRAMES)
    *run(i) = *reinterpret_cast<const float4*>(i >= A.M ? stage[1][i - A.M] : stage[0][i]);
}

}  // namespace mi355tts
