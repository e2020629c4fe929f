// mi355tts host runtime — pitch: the load, frame-count and call entry points (kernel: pitch.h)
// (one translation unit: included once by mi355tts.hip, after limiter_forward.h; the call frame, the model table and the
// waveform intake: host_call.h; RowWriter: host_rows.h)
#pragma once

constexpr int PT_MAX_SAMPLES_LOG2 = 30;
constexpr int PT_MAX_HOP = 4096;

extern "C" int mi355tts_load_pitch(mi355tts_ctx* ctx, const mi355tts_pitch_params* params, int* model_out) {
  if (!ctx || !params || !model_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  const mi355tts_pitch_params& p = *params;
  if (p.sample_rate < 1 || p.sample_rate > (1 << 24)) return fail(MI355TTS_ERR_INVALID, "sample_rate %d outside [1, 2^24]", p.sample_rate);
  if (p.hop < 1 || p.hop > PT_MAX_HOP) return fail(MI355TTS_ERR_INVALID, "hop %d outside [1, %d]", p.hop, PT_MAX_HOP);
  if (p.window < 64 || p.window > PT_MAX_W || p.window % 4) return fail(MI355TTS_ERR_INVALID, "window %d is not a multiple of 4 in [64, %d]", p.window, PT_MAX_W);
  if (p.tau_min < 1 || p.tau_min > p.tau_max || p.tau_max > PT_MAX_TAU)
    return fail(MI355TTS_ERR_INVALID, "tau_min %d / tau_max %d: 1 <= tau_min <= tau_max <= %d", p.tau_min, p.tau_max, PT_MAX_TAU);
  if (p.window + p.tau_max > PT_SPAN) return fail(MI355TTS_ERR_INVALID, "window %d + tau_max %d > %d", p.window, p.tau_max, PT_SPAN);
  if (!(p.threshold > 0.f && p.threshold <= 1.f)) return fail(MI355TTS_ERR_INVALID, "threshold %g outside (0, 1]", (double)p.threshold);
  auto pm = std::make_shared<PitchModel>();
  pm->p = p;
  return register_model(ctx, std::move(pm), model_out);
}

extern "C" int64_t mi355tts_pitch_frames(mi355tts_ctx* ctx, int model, int64_t samples) {
  if (!ctx) return fail(MI355TTS_ERR_INVALID, "null argument");
  std::shared_ptr<PitchModel> pin;
  CHECK(find_model(ctx, model, &pin));
  if (samples < 0 || samples > (1LL << PT_MAX_SAMPLES_LOG2)) return fail(MI355TTS_ERR_INVALID, "samples %lld outside [0, 2^%d]", (long long)samples, PT_MAX_SAMPLES_LOG2);
  return samples / pin->p.hop;
}

template <bool I16>
static void pitch_launch(int nk, dim3 grid, hipStream_t s, const PitchArgs& a) {
  const dim3 tb(PT_THREADS);
  if (nk == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(pitch_kernel<I16, 1>), grid, tb, 0, s, a);
  else if (nk == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(pitch_kernel<I16, 2>), grid, tb, 0, s, a);
  else if (nk == 3) hipLaunchKernelGGL(HIP_KERNEL_NAME(pitch_kernel<I16, 3>), grid, tb, 0, s, a);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(pitch_kernel<I16, 4>), grid, tb, 0, s, a);
}

// pitch_kernel on the rows `a` names (the input, the planes and their stride a.ld bound by the caller): ONE launch, a.ld columns
// x B rows, `total` frames in all.  (shift_forward.h queues the same launch for the periods of its rows.)
static void pitch_enqueue(mi355tts_ctx* ctx, Worker* w, hipStream_t s, const mi355tts_pitch_params& p, PitchArgs& a, bool in_i16, int B,
                          long long total) {
  a.hop = p.hop;
  a.W = p.window;
  a.tau_min = p.tau_min;
  a.tau_max = p.tau_max;
  a.interpolate = p.interpolate != 0;
  a.sample_rate = (float)p.sample_rate;
  a.theta = p.threshold;
  ProfScope ps(ctx, w, KC_SMALL, 3.0 * (double)total * p.window * p.tau_max);
  ps.kernel(KN_PITCH);
  const dim3 grid((unsigned)a.ld, B);
  const int nk = (p.tau_max + PT_THREADS - 1) / PT_THREADS;
  if (in_i16) pitch_launch<true>(nk, grid, s, a);
  else pitch_launch<false>(nk, grid, s, a);
}

extern "C" int mi355tts_pitch(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                              int64_t in_ld, float* f0_out, float* periodicity_out, float* level_db_out, float* cmnd_out, int64_t out_ld,
                              uint32_t flags) {
  if (!ctx || !samples) return fail(MI355TTS_ERR_INVALID, "null argument");
  if ((in_f32 != nullptr) == (in_i16 != nullptr)) return fail(MI355TTS_ERR_INVALID, "exactly one of in_f32 / in_i16 must be given");
  if (B <= 0 || B > 65535 || in_ld < 0) return fail(MI355TTS_ERR_INVALID, "batch outside [1, 65535] or negative in_ld");
  if (!f0_out && !periodicity_out && !level_db_out) return fail(MI355TTS_ERR_INVALID, "no output: give f0_out, periodicity_out or level_db_out");
  std::shared_ptr<PitchModel> pin;
  CHECK(find_model(ctx, model, &pin));
  const mi355tts_pitch_params& p = pin->p;
  WaveIn in{in_f32, in_i16, samples, B, in_ld, (flags & MI355TTS_IN_DEVICE) != 0};
  CHECK(in.check("in_ld", PT_MAX_SAMPLES_LOG2));
  const bool out_dev = (flags & MI355TTS_OUT_DEVICE) != 0;
  long long Fmax = 0, total = 0;
  for (int b = 0; b < B; ++b) {
    Fmax = std::max(Fmax, (long long)(samples[b] / p.hop));
    total += samples[b] / p.hop;
  }
  if (out_ld > INT_MAX) return fail(MI355TTS_ERR_INVALID, "out_ld %lld > 2^31 - 1", (long long)out_ld);
  if (out_ld < Fmax) return fail(MI355TTS_ERR_INVALID, "out_ld %lld < %lld frames of the longest row", (long long)out_ld, Fmax);
  const size_t T1 = (size_t)p.tau_max + 1;
  float* const planes[3] = {f0_out, periodicity_out, level_db_out};
  CallFrame f(ctx);
  CHECK(f.open());
  Worker* w = f.w;
  hipStream_t s = f.s;
  const RowWriter wr{out_dev, s};
  if (Fmax == 0) {  // no frame in any row: zeros, and no launch
    for (float* pl : planes)
      if (pl) CHECK(wr.zero(pl, (size_t)B * (size_t)out_ld));
    if (cmnd_out) CHECK(wr.zero(cmnd_out, (size_t)B * (size_t)out_ld * T1));
    if (out_dev) return f.finish();
    f.done = true;
    return 0;
  }
  CHECK(f.pinned_ints((size_t)B));
  // host outputs: planes [B][Fmax] and the d' rows [B][Fmax][T1] in the workspace, then in the pinned staging behind the staged
  // input; device outputs are written in place, at the caller's stride, zeros behind the rows' frames included
  const size_t ld = out_dev ? (size_t)out_ld : (size_t)Fmax;
  const size_t plane_b = sizeof(float) * (size_t)B * ld, cmnd_b = plane_b * T1;
  Carver cv;
  in.carve(cv);
  size_t o_plane[3] = {}, o_cmnd = 0, host_b = 0;
  if (!out_dev) {
    for (int k = 0; k < 3; ++k)
      if (planes[k]) {
        o_plane[k] = cv.take(plane_b);
        host_b += plane_b;
      }
    if (cmnd_out) {
      o_cmnd = cv.take(cmnd_b);
      host_b += cmnd_b;
    }
  }
  CHECK(f.reserve(cv.pos, in.bytes + host_b));
  CHECK(in.upload(f, w->pinned));
  char* base = w->arena;
  PitchArgs a;
  std::memset(&a, 0, sizeof(a));
  in.bind(a);
  a.ld = (long long)ld;
  float** const dst[3] = {&a.f0, &a.per, &a.lvl};
  for (int k = 0; k < 3; ++k) *dst[k] = !planes[k] ? nullptr : out_dev ? planes[k] : (float*)(base + o_plane[k]);
  a.cmnd = !cmnd_out ? nullptr : out_dev ? cmnd_out : (float*)(base + o_cmnd);
  pitch_enqueue(ctx, w, s, p, a, in_i16 != nullptr, B, total);
  if (out_dev) return f.finish();
  char* pin_out = w->pinned_out + in.bytes;
  size_t at = 0;
  for (int k = 0; k < 3; ++k)
    if (planes[k]) {
      HIPCHECK(hipMemcpyAsync(pin_out + at, *dst[k], plane_b, hipMemcpyDeviceToHost, s));
      at += plane_b;
    }
  if (cmnd_out) HIPCHECK(hipMemcpyAsync(pin_out + at, a.cmnd, cmnd_b, hipMemcpyDeviceToHost, s));
  CHECK(f.finish());
  // staging rows of Fmax columns -> the caller's rows of out_ld columns (the kernel wrote the zeros up to Fmax)
  auto scatter = [&](float* out, const char* src, size_t per) {
    for (int b = 0; b < B; ++b) {
      float* row = out + (size_t)b * (size_t)out_ld * per;
      std::memcpy(row, src + sizeof(float) * (size_t)b * ld * per, sizeof(float) * ld * per);
      std::memset(row + ld * per, 0, sizeof(float) * ((size_t)out_ld - ld) * per);
    }
  };
  at = 0;
  for (int k = 0; k < 3; ++k)
    if (planes[k]) {
      scatter(planes[k], pin_out + at, 1);
      at += plane_b;
    }
  if (cmnd_out) scatter(cmnd_out, pin_out + at, T1);
  return 0;
}
