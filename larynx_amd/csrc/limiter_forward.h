// mi355tts host runtime — limiter: the load and call entry points (kernels: limiter.h)
// (one translation unit: included once by mi355tts.hip, after loudness_forward.h; the model table, pack_polyphase and upload:
// host_call.h; the frame of the call, WaveCall, and the row delivery: host_rows.h)
#pragma once

constexpr int LM_MAX_SAMPLES_LOG2 = 24;

extern "C" int mi355tts_load_limiter(mi355tts_ctx* ctx, const mi355tts_limiter_params* params, const float* taps, const float* window,
                                     int* model_out) {
  if (!ctx || !params || !window || !model_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  const int os = params->oversample, la = params->lookahead;
  if (os < 1 || os > LM_MAX_OS) return fail(MI355TTS_ERR_INVALID, "oversample %d outside [1, %d]", os, LM_MAX_OS);
  if (la < 0 || la > LM_MAX_LA) return fail(MI355TTS_ERR_INVALID, "lookahead %d outside [0, %d]", la, LM_MAX_LA);
  if (!(params->release >= 0.f && params->release < 1.f)) return fail(MI355TTS_ERR_INVALID, "release %g outside [0, 1)", (double)params->release);
  if (os > 1 && !taps) return fail(MI355TTS_ERR_INVALID, "null argument");  // (with oversample 1 no taps are read)
  auto lm = std::make_shared<LimiterModel>();
  std::vector<float> table;  // as a resampler's with up = os
  if (os > 1) CHECK(pack_polyphase(taps, params->half_len, os, LM_MAX_T, &lm->T, &lm->Tp, table));
  double wsum = 0;
  for (int j = 0; j <= la; ++j) {
    if (!std::isfinite(window[j])) return fail(MI355TTS_ERR_INVALID, "window[%d] is not finite", j);
    if (window[j] < 0.f) return fail(MI355TTS_ERR_INVALID, "window[%d] = %g is negative", j, (double)window[j]);
    wsum += (double)window[j];
  }
  if (!(std::fabs(wsum - 1.0) <= 1e-6)) return fail(MI355TTS_ERR_INVALID, "window sums to %.9g, not to 1 within 1e-6", wsum);
  lm->p = *params;
  lm->device = ctx->device;
  HIPCHECK(hipSetDevice(ctx->device));
  if (os > 1) CHECK(upload(&lm->table, table, "limiter table"));
  CHECK(upload(&lm->win, std::vector<float>(window, window + la + 1), "limiter window"));
  std::vector<float> pw((size_t)LM_GROUP + 1);
  for (int k = 0; k <= LM_GROUP; ++k) pw[k] = (float)std::pow((double)params->release, (double)k);  // (pow(0, 0) = 1)
  CHECK(upload(&lm->pw, pw, "limiter powers"));
  return register_model(ctx, std::move(lm), model_out);
}

extern "C" int mi355tts_limit(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                              int64_t in_ld, const float* gain, float ceiling, float* out_f32, int16_t* out_i16, int64_t out_ld,
                              float* true_peak_out, float* min_gain_out, float* curve_out, uint32_t flags) {
  WaveCall wc(ctx, in_f32, in_i16, samples, B, in_ld, out_f32, out_i16, out_ld, flags);
  CHECK(wc.check_args());
  if (!(ceiling > 0.f && ceiling <= 1.f)) return fail(MI355TTS_ERR_INVALID, "ceiling %g outside (0, 1]", (double)ceiling);
  if (gain)
    for (int b = 0; b < B; ++b)
      if (!std::isfinite(gain[b]) || gain[b] < 0.f) return fail(MI355TTS_ERR_INVALID, "gain[%d] = %g is not a finite value >= 0", b, (double)gain[b]);
  std::shared_ptr<LimiterModel> pin;
  CHECK(find_model(ctx, model, &pin));
  const LimiterModel* lm = pin.get();
  CHECK(wc.in.check("in_ld", LM_MAX_SAMPLES_LOG2));
  const long long Nmax = wc.in.Nmax;
  CHECK(wc.check_out(Nmax));
  const bool any_out = out_f32 || out_i16;
  const bool meter = !any_out && !curve_out;  // a meter call: the two launches TP needs
  CHECK(wc.open(curve_out, {true_peak_out, min_gain_out}));  // the side plane: the gain curve
  Worker* w = wc.f.w;
  hipStream_t s = wc.f.s;
  if (Nmax == 0) return wc.empty({0.f, 1.f});  // nothing in any row: true peak 0, gain 1
  CHECK(wc.f.pinned_ints(2 * (size_t)B));  // the sample counts, then the gains
  const int la = lm->p.lookahead;
  const size_t Nld = wc.in.Nld;
  const long long tiles = (Nmax + LM_TILE - 1) / LM_TILE;
  const int gmax = (int)((Nmax + la + LM_GROUP - 1) / LM_GROUP);
  Carver cv = wc.carve();
  const size_t o_gain = cv.take(sizeof(float) * (size_t)B);
  const size_t o_tp = cv.take(sizeof(float) * (size_t)B * tiles);
  const size_t o_c = cv.take(meter ? 0 : sizeof(float) * (size_t)B * Nld);
  const size_t o_tm = cv.take(meter ? 0 : sizeof(float) * (size_t)B * tiles);
  const size_t o_dg = cv.take(meter ? 0 : sizeof(float) * (size_t)B * gmax * LM_GROUP);
  const size_t o_gs = cv.take(meter ? 0 : sizeof(float) * (size_t)B * gmax);
  CHECK(wc.reserve(cv));
  char* base = w->arena;
  float* const h_gain = reinterpret_cast<float*>(w->pinned + B);
  for (int b = 0; b < B; ++b) h_gain[b] = gain ? gain[b] : 1.f;
  HIPCHECK(hipMemcpyAsync(base + o_gain, h_gain, sizeof(float) * B, hipMemcpyHostToDevice, s));
  LimiterArgs a;
  std::memset(&a, 0, sizeof(a));
  wc.in.bind(a);
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
  a.res = wc.d_res;
  a.gmax = gmax;
  if (!meter) {
    a.c = (float*)(base + o_c);
    a.c_bs = (long long)Nld;
    a.tmin = (float*)(base + o_tm);
    a.dg = (float*)(base + o_dg);
    a.gs = (float*)(base + o_gs);
  }
  const long long total = wc.in.total;
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
    const long long ld = wc.ld;
    a.y = wc.d_y;
    a.pcm = wc.d_pcm;
    a.y_bs = a.y_ld = a.pcm_bs = a.pcm_ld = ld;
    if (curve_out) {
      a.curve = wc.d_side;
      a.curve_bs = a.curve_ld = wc.side_ld;
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
  CHECK(wc.end());
  if (meter && min_gain_out) std::fill_n(min_gain_out, B, 1.f);  // (no curve was made: nothing reduced any gain)
  return 0;
}
