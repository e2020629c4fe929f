// mi355tts host runtime — limiter: the load and call entry points (kernels: limiter.h)
// (one translation unit: included once by mi355tts.hip, after loudness_forward.h; the call frame, the model table and the
// waveform intake: host_call.h; the row delivery: hifigan_forward.h)
#pragma once

constexpr int LM_MAX_SAMPLES_LOG2 = 24;

extern "C" int mi355tts_load_limiter(mi355tts_ctx* ctx, const mi355tts_limiter_params* params, const float* taps, const float* window,
                                     int* model_out) {
  if (!ctx || !params || !window || !model_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  const int os = params->oversample, la = params->lookahead;
  if (os < 1 || os > LM_MAX_OS) return fail(MI355TTS_ERR_INVALID, "oversample %d outside [1, %d]", os, LM_MAX_OS);
  if (la < 0 || la > LM_MAX_LA) return fail(MI355TTS_ERR_INVALID, "lookahead %d outside [0, %d]", la, LM_MAX_LA);
  if (!(params->release >= 0.f && params->release < 1.f)) return fail(MI355TTS_ERR_INVALID, "release %g outside [0, 1)", (double)params->release);
  long long ntaps = 0, T = 0;
  if (os > 1) {  // (with oversample 1 no taps are read)
    if (!taps) return fail(MI355TTS_ERR_INVALID, "null argument");
    if (params->half_len < 0) return fail(MI355TTS_ERR_INVALID, "half_len %d < 0", params->half_len);
    ntaps = 2LL * params->half_len + 1;
    T = (ntaps + os - 1) / os;
    if (T > LM_MAX_T) return fail(MI355TTS_ERR_INVALID, "%lld taps per phase > %d", T, LM_MAX_T);
    for (long long j = 0; j < ntaps; ++j)
      if (!std::isfinite(taps[j])) return fail(MI355TTS_ERR_INVALID, "tap %lld is not finite", j);
  }
  double wsum = 0;
  for (int j = 0; j <= la; ++j) {
    if (!std::isfinite(window[j])) return fail(MI355TTS_ERR_INVALID, "window[%d] is not finite", j);
    if (window[j] < 0.f) return fail(MI355TTS_ERR_INVALID, "window[%d] = %g is negative", j, (double)window[j]);
    wsum += (double)window[j];
  }
  if (!(std::fabs(wsum - 1.0) <= 1e-6)) return fail(MI355TTS_ERR_INVALID, "window sums to %.9g, not to 1 within 1e-6", wsum);
  auto lm = std::make_shared<LimiterModel>();
  lm->p = *params;
  lm->device = ctx->device;
  HIPCHECK(hipSetDevice(ctx->device));
  auto upload = [&](float** dst, const std::vector<float>& v, const char* what) -> int {
    if (hipMalloc(dst, v.size() * sizeof(float)) != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc limiter %s", what);
    HIPCHECK(hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
  };
  if (os > 1) {
    lm->T = (int)T;
    lm->Tp = ((int)T + 3) & ~3;
    std::vector<float> table((size_t)os * lm->Tp, 0.f);  // [p][t] = taps[p + t * os], as a resampler's with up = os
    for (long long j = 0; j < ntaps; ++j) table[(size_t)(j % os) * lm->Tp + (size_t)(j / os)] = taps[j];
    CHECK(upload(&lm->table, table, "table"));
  }
  CHECK(upload(&lm->win, std::vector<float>(window, window + la + 1), "window"));
  std::vector<float> pw((size_t)LM_GROUP + 1);
  for (int k = 0; k <= LM_GROUP; ++k) pw[k] = (float)std::pow((double)params->release, (double)k);  // (pow(0, 0) = 1)
  CHECK(upload(&lm->pw, pw, "powers"));
  return register_model(ctx, std::move(lm), model_out);
}

extern "C" int mi355tts_limit(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                              int64_t in_ld, const float* gain, float ceiling, float* out_f32, int16_t* out_i16, int64_t out_ld,
                              float* true_peak_out, float* min_gain_out, float* curve_out, uint32_t flags) {
  if (!ctx || !samples) return fail(MI355TTS_ERR_INVALID, "null argument");
  if ((in_f32 != nullptr) == (in_i16 != nullptr)) return fail(MI355TTS_ERR_INVALID, "exactly one of in_f32 / in_i16 must be given");
  if (B <= 0 || in_ld < 0) return fail(MI355TTS_ERR_INVALID, "empty batch or negative in_ld");
  if (!(ceiling > 0.f && ceiling <= 1.f)) return fail(MI355TTS_ERR_INVALID, "ceiling %g outside (0, 1]", (double)ceiling);
  if (gain)
    for (int b = 0; b < B; ++b)
      if (!std::isfinite(gain[b]) || gain[b] < 0.f) return fail(MI355TTS_ERR_INVALID, "gain[%d] = %g is not a finite value >= 0", b, (double)gain[b]);
  std::shared_ptr<LimiterModel> pin;
  CHECK(find_model(ctx, model, &pin));
  const LimiterModel* lm = pin.get();
  WaveIn in{in_f32, in_i16, samples, B, in_ld, (flags & MI355TTS_IN_DEVICE) != 0};
  CHECK(in.check("in_ld", LM_MAX_SAMPLES_LOG2));
  const long long Nmax = in.Nmax;
  const bool any_out = out_f32 || out_i16;
  if (any_out && out_ld < Nmax) return fail(MI355TTS_ERR_INVALID, "out_ld %lld < %lld samples of the longest row", (long long)out_ld, Nmax);
  const bool meter = !any_out && !curve_out;  // a meter call: the two launches TP needs
  const bool out_dev = (flags & MI355TTS_OUT_DEVICE) != 0;
  CallFrame f(ctx);
  CHECK(f.open());
  Worker* w = f.w;
  hipStream_t s = f.s;
  const OutRows rows = {nullptr, nullptr, 0, {out_f32, out_i16, out_ld, 0, 0, (size_t)Nmax}};
  if (Nmax == 0) {  // nothing in any row: true peak 0, gain 1, every output zero
    for (int b = 0; b < B; ++b) {
      if (true_peak_out) true_peak_out[b] = 0.f;
      if (min_gain_out) min_gain_out[b] = 1.f;
    }
    if (curve_out) CHECK((RowWriter{out_dev, s}).zero(curve_out, (size_t)B * (size_t)in_ld));
    return zero_outputs(f, rows, B, out_dev);
  }
  CHECK(f.pinned_ints(2 * (size_t)B));  // the sample counts, then the gains
  const int la = lm->p.lookahead;
  const size_t Nld = (size_t)((Nmax + 7) & ~7LL);
  const long long tiles = (Nmax + LM_TILE - 1) / LM_TILE;
  const int gmax = (int)((Nmax + la + LM_GROUP - 1) / LM_GROUP);
  const bool curve_direct = curve_out && out_dev;
  Carver cv;
  in.carve(cv);
  const size_t o_gain = cv.take(sizeof(float) * (size_t)B);
  const size_t o_tp = cv.take(sizeof(float) * (size_t)B * tiles);
  const size_t o_res = cv.take(sizeof(float) * 2 * (size_t)B);
  const size_t o_c = cv.take(meter ? 0 : sizeof(float) * (size_t)B * Nld);
  const size_t o_tm = cv.take(meter ? 0 : sizeof(float) * (size_t)B * tiles);
  const size_t o_dg = cv.take(meter ? 0 : sizeof(float) * (size_t)B * gmax * LM_GROUP);
  const size_t o_gs = cv.take(meter ? 0 : sizeof(float) * (size_t)B * gmax);
  const size_t o_curve = cv.take(curve_out && !curve_direct ? sizeof(float) * (size_t)B * Nld : 0);
  const size_t o_y = cv.take(out_f32 && !out_dev ? sizeof(float) * (size_t)B * Nld : 0);
  const size_t o_pcm = cv.take(out_i16 && !out_dev ? sizeof(short) * (size_t)B * Nld : 0);
  // host outputs wait in the pinned staging behind the staged input: the delivered rows and the per-row results, then the curve
  const Staging st = host_staging(B, out_f32 && !out_dev, Nld, out_i16 && !out_dev, Nld, in.bytes, sizeof(float) * 2 * (size_t)B);
  const size_t curve_host = curve_out && !out_dev ? sizeof(float) * (size_t)B * Nld : 0;
  CHECK(f.reserve(cv.pos, st.end() + curve_host));
  char* base = w->arena;
  CHECK(in.upload(f, w->pinned));
  float* const h_gain = reinterpret_cast<float*>(w->pinned + B);
  for (int b = 0; b < B; ++b) h_gain[b] = gain ? gain[b] : 1.f;
  HIPCHECK(hipMemcpyAsync(base + o_gain, h_gain, sizeof(float) * B, hipMemcpyHostToDevice, s));
  LimiterArgs a;
  std::memset(&a, 0, sizeof(a));
  a.in_f32 = in_f32 ? (const float*)in.d : nullptr;
  a.in_i16 = in_i16 ? (const short*)in.d : nullptr;
  a.in_bs = in.bs;
  a.samples = in.d_samples;
  a.gain = (const float*)(base + o_gain);
  a.ceiling = ceiling;
  a.os = lm->p.oversample;
  a.half_len = lm->p.half_len;
  a.Tp = lm->Tp;
  a.table = lm->table;
  a.la = la;
  a.win = lm->win;
  a.pw = lm->pw;
  a.tpeak = (float*)(base + o_tp);
  a.t_ld = tiles;
  a.res = (float*)(base + o_res);
  a.gmax = gmax;
  if (!meter) {
    a.c = (float*)(base + o_c);
    a.c_bs = (long long)Nld;
    a.tmin = (float*)(base + o_tm);
    a.dg = (float*)(base + o_dg);
    a.gs = (float*)(base + o_gs);
  }
  long long total = 0;
  for (int b = 0; b < B; ++b) total += samples[b];
  const dim3 tb(LM_THREADS);
  {
    ProfScope ps(ctx, w, KC_SMALL, 2.0 * (double)total * (a.os > 1 ? a.os * lm->T : 0));
    ps.kernel(KN_LIM_PEAK);
    if (in_i16) hipLaunchKernelGGL(limiter_peak_kernel<true>, dim3((unsigned)tiles, B), tb, 0, s, a);
    else hipLaunchKernelGGL(limiter_peak_kernel<false>, dim3((unsigned)tiles, B), tb, 0, s, a);
  }
  {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    ps.kernel(KN_LIM_REDUCE);
    hipLaunchKernelGGL(limiter_reduce_kernel<false>, dim3(B), tb, 0, s, a);
  }
  float* d_y = nullptr;
  short* d_pcm = nullptr;
  if (!meter) {
    {
      ProfScope ps(ctx, w, KC_SMALL, 0);
      ps.kernel(KN_LIM_HOLD);
      hipLaunchKernelGGL(limiter_hold_kernel, dim3(gmax, B), tb, 0, s, a);
    }
    {
      ProfScope ps(ctx, w, KC_SMALL, 0);
      ps.kernel(KN_LIM_CARRY);
      hipLaunchKernelGGL(limiter_carry_kernel, dim3(B), tb, 0, s, a);
    }
    const long long ld = out_dev ? (long long)out_ld : (long long)Nld;
    d_y = !out_f32 ? nullptr : out_dev ? out_f32 : (float*)(base + o_y);
    d_pcm = !out_i16 ? nullptr : out_dev ? (short*)out_i16 : (short*)(base + o_pcm);
    a.y = d_y;
    a.pcm = d_pcm;
    a.y_bs = a.y_ld = a.pcm_bs = a.pcm_ld = ld;
    if (curve_out) {
      a.curve = curve_direct ? curve_out : (float*)(base + o_curve);
      a.curve_bs = a.curve_ld = curve_direct ? (long long)in_ld : (long long)Nld;
    }
    {
      // (the grid also covers the zero tails of the rows the caller's device buffers hold: up to their strides)
      const long long span = std::max(std::max(any_out ? ld : 0LL, a.curve ? a.curve_ld : 0LL), Nmax);
      ProfScope ps(ctx, w, KC_SMALL, 2.0 * (double)total * (la + 1));
      ps.kernel(KN_LIM_APPLY);
      const dim3 grid((unsigned)((span + LM_TILE - 1) / LM_TILE), B);
      if (in_i16) hipLaunchKernelGGL(limiter_apply_kernel<true>, grid, tb, 0, s, a);
      else hipLaunchKernelGGL(limiter_apply_kernel<false>, grid, tb, 0, s, a);
    }
    {
      ProfScope ps(ctx, w, KC_SMALL, 0);
      ps.kernel(KN_LIM_REDUCE);
      hipLaunchKernelGGL(limiter_reduce_kernel<true>, dim3(B), tb, 0, s, a);
    }
  }
  char* const pc_host = w->pinned_out + st.end();
  if (curve_host) HIPCHECK(hipMemcpyAsync(pc_host, a.curve, curve_host, hipMemcpyDeviceToHost, s));
  std::vector<float> res((size_t)2 * B);
  // (with device outputs the staging holds no rows: the per-row results alone travel, and scatter_rows finds nothing to write)
  const OutRows host_rows = out_dev ? OutRows{nullptr, nullptr, 0, {nullptr, nullptr, 0, 0, 0, 0}} : rows;
  CHECK(deliver_rows(f, host_rows, B, WavRows{d_y, Nld, d_pcm, Nld}, st, true, res.data(), a.res));
  for (int b = 0; b < B; ++b) {
    if (true_peak_out) true_peak_out[b] = res[2 * b];
    if (min_gain_out) min_gain_out[b] = meter ? 1.f : res[2 * b + 1];
    if (curve_host) {
      float* dst = curve_out + (size_t)b * (size_t)in_ld;
      std::memcpy(dst, pc_host + sizeof(float) * (size_t)b * Nld, sizeof(float) * (size_t)samples[b]);
      std::memset(dst + samples[b], 0, sizeof(float) * ((size_t)in_ld - (size_t)samples[b]));
    }
  }
  return 0;
}
