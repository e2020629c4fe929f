// mi355tts host runtime — pitch shift and tempo: the load, length and call entry points (kernels: shift.h; the periods:
// pitch_enqueue of pitch_forward.h; the playback: resample_launch / resample_pcm_launch of resample_forward.h)
// (one translation unit: included once by mi355tts.hip, after pitch_forward.h; the frame of the call, WaveCall: host_rows.h)
#pragma once

static_assert(SH_PEAK_TILE == RS_TILE, "shift_ola_kernel leaves its peaks in resample_pcm_kernel's tiles");

static long long shift_stretched(const ShiftModel* sm, long long n) { return (n * sm->p.up + sm->p.down - 1) / sm->p.down; }
static long long shift_frames(const ShiftModel* sm, long long L) { return L > 0 ? (L - 1) / (sm->p.window / 2) + 2 : 0; }
static long long shift_delivered(const ShiftModel* sm, long long n) { return sm->resampler ? n : shift_stretched(sm, n); }

extern "C" int mi355tts_load_shift(mi355tts_ctx* ctx, const mi355tts_shift_params* params, const float* window, int* model_out) {
  if (!ctx || !params || !window || !model_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  const mi355tts_shift_params& p = *params;
  if (p.up < 1 || p.up > SH_MAX_UD || p.down < 1 || p.down > SH_MAX_UD)
    return fail(MI355TTS_ERR_INVALID, "up %d / down %d outside [1, %d]", p.up, p.down, SH_MAX_UD);
  int g = p.up;
  for (int r = p.down; r;) {
    const int t = g % r;
    g = r;
    r = t;
  }
  if (g != 1) return fail(MI355TTS_ERR_INVALID, "up %d and down %d are not coprime", p.up, p.down);
  if (p.window < 64 || p.window > SH_MAX_N || p.window % 4) return fail(MI355TTS_ERR_INVALID, "window %d is not a multiple of 4 in [64, %d]", p.window, SH_MAX_N);
  for (int i = 0; i < p.window; ++i)
    if (!std::isfinite(window[i])) return fail(MI355TTS_ERR_INVALID, "window value %d is not finite", i);
  auto sm = std::make_shared<ShiftModel>();
  sm->p = p;
  sm->device = ctx->device;
  CHECK(find_model(ctx, p.pitch, &sm->pitch));
  if (p.resampler != 0) {
    CHECK(find_model(ctx, p.resampler, &sm->resampler));
    const mi355tts_resampler_params& r = sm->resampler->p;
    if (p.up == p.down) return fail(MI355TTS_ERR_INVALID, "up == down leaves nothing to resample: no resampler with the ratio 1 / 1");
    if (r.up != p.down || r.down != p.up)
      return fail(MI355TTS_ERR_INVALID, "the resampler's ratio %d / %d is not down / up = %d / %d", r.up, r.down, p.down, p.up);
  }
  HIPCHECK(hipSetDevice(ctx->device));
  CHECK(upload(&sm->win, std::vector<float>(window, window + p.window), "shift window"));
  return register_model(ctx, std::move(sm), model_out);
}

extern "C" int64_t mi355tts_shift_length(mi355tts_ctx* ctx, int model, int64_t samples) {
  if (!ctx) return fail(MI355TTS_ERR_INVALID, "null argument");
  std::shared_ptr<ShiftModel> pin;
  CHECK(find_model(ctx, model, &pin));
  if (samples < 0 || samples > RS_MAX_SAMPLES) return fail(MI355TTS_ERR_INVALID, "samples %lld outside [0, 2^24]", (long long)samples);
  return shift_delivered(pin.get(), samples);
}

extern "C" int mi355tts_shift(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                              int64_t in_ld, const int32_t* positions_in, float* out_f32, int16_t* out_i16, int64_t out_ld, int pcm_mode,
                              int32_t* positions_out, int64_t pos_ld, float* f0_out, int64_t f0_ld, int64_t* samples_out, uint32_t flags) {
  WaveCall wc(ctx, in_f32, in_i16, samples, B, in_ld, out_f32, out_i16, out_ld, flags);
  CHECK(wc.check_args());
  if (!out_f32 && !out_i16) return fail(MI355TTS_ERR_INVALID, "no output: give out_f32, out_i16 or both");
  if (pcm_mode != MI355TTS_PCM_SATURATE && pcm_mode != MI355TTS_PCM_NORMALIZE) return fail(MI355TTS_ERR_INVALID, "unknown pcm_mode %d", pcm_mode);
  if (positions_in && (positions_out || f0_out))
    return fail(MI355TTS_ERR_INVALID, "positions_in replaces the periods and the positions: no positions_out / f0_out with it");
  std::shared_ptr<ShiftModel> pin;
  CHECK(find_model(ctx, model, &pin));
  const ShiftModel* sm = pin.get();
  const mi355tts_pitch_params& pp = sm->pitch->p;
  const bool pitch_mode = sm->resampler != nullptr;
  CHECK(wc.in.check("in_ld", RS_MAX_SAMPLES_LOG2));
  long long Lmax = 0, Kmax = 0, Fmax = 0, Omax = 0, Ltotal = 0, Ftotal = 0, Ototal = 0;
  for (int b = 0; b < B; ++b) {
    const long long L = shift_stretched(sm, samples[b]), F = samples[b] / pp.hop, O = shift_delivered(sm, samples[b]);
    Lmax = std::max(Lmax, L);
    Kmax = std::max(Kmax, shift_frames(sm, L));
    Fmax = std::max(Fmax, F);
    Omax = std::max(Omax, O);
    Ltotal += L;
    Ftotal += F;
    Ototal += O;
  }
  CHECK(wc.check_out(Omax));
  if ((positions_in || positions_out) && pos_ld < Kmax)
    return fail(MI355TTS_ERR_INVALID, "pos_ld %lld < %lld frames of the longest row", (long long)pos_ld, Kmax);
  if (f0_out && f0_ld < Fmax) return fail(MI355TTS_ERR_INVALID, "f0_ld %lld < %lld pitch frames of the longest row", (long long)f0_ld, Fmax);
  if (samples_out)
    for (int b = 0; b < B; ++b) samples_out[b] = shift_delivered(sm, samples[b]);
  const bool normalize = out_i16 && pcm_mode == MI355TTS_PCM_NORMALIZE;
  const bool in_dev = wc.in.in_dev, out_dev = wc.out_dev;
  CHECK(wc.open());
  Worker* w = wc.f.w;
  hipStream_t s = wc.f.s;
  const RowWriter wr{out_dev, s};
  if (Omax == 0) {  // no sample in any row: no frame either
    if (positions_out) CHECK(wr.zero(positions_out, (size_t)B * (size_t)pos_ld));
    if (f0_out) CHECK(wr.zero(f0_out, (size_t)B * (size_t)f0_ld));
    return wc.empty({});
  }
  CHECK(wc.f.pinned_ints(2 * (size_t)B));
  // ---- the workspace: the input | the stretched lengths | f0 | positions | the stretched rows (PITCH) | what the delivery takes.
  // Device planes of the caller (f0_out, positions_out, positions_in) are written and read in place, at the caller's stride.
  const bool run_pitch = !positions_in && Fmax > 0;
  const bool f0_direct = f0_out && out_dev, pos_direct = positions_in ? in_dev : positions_out && out_dev;
  const size_t f0_ldw = f0_direct ? (size_t)f0_ld : (size_t)Fmax, pos_ldw = pos_direct ? (size_t)pos_ld : (size_t)Kmax;
  const size_t Lld = (size_t)((Lmax + 7) & ~7LL);
  const size_t f0_b = sizeof(float) * (size_t)B * (size_t)Fmax, pos_b = sizeof(int) * (size_t)B * (size_t)Kmax;
  const WaveOutPlan plan = wave_out_plan(out_f32, out_i16, normalize, Omax);
  Carver cv = wc.carve();
  const size_t o_L = cv.take(sizeof(int) * (size_t)B);
  const size_t o_f0 = cv.take(run_pitch && !f0_direct ? f0_b : 0);
  const size_t o_pos = cv.take(pos_direct ? 0 : pos_b);
  const size_t o_ys = cv.take(pitch_mode ? sizeof(float) * (size_t)B * Lld : 0);
  const WaveOutTakes tk = wave_out_carve(cv, wc, plan);
  // pinned staging of this stage's own: host positions on their way in or out, then the host f0 plane
  const size_t pos_host = (positions_in && !in_dev) || (positions_out && !out_dev) ? pos_b : 0;
  const size_t f0_host = f0_out && !out_dev && run_pitch ? f0_b : 0;
  wc.extra_host = pos_host + f0_host;
  CHECK(wc.reserve(cv));
  char* base = w->arena;
  char* const p_pos = w->pinned_out + wc.extra_at();
  char* const p_f0 = p_pos + pos_host;
  int* const d_L = (int*)(base + o_L);
  {
    int* Lh = w->pinned + B;
    for (int b = 0; b < B; ++b) Lh[b] = (int)shift_stretched(sm, samples[b]);
    HIPCHECK(hipMemcpyAsync(d_L, Lh, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, s));
  }
  float* const d_f0 = !run_pitch ? nullptr : f0_direct ? f0_out : (float*)(base + o_f0);
  int* d_pos = pos_direct ? (positions_in ? const_cast<int32_t*>(positions_in) : positions_out) : (int*)(base + o_pos);
  if (f0_out && !run_pitch && out_dev) CHECK(wr.zero(f0_out, (size_t)B * (size_t)f0_ld));  // (no pitch frame in any row)
  if (positions_in && !in_dev) {  // the caller's rows of pos_ld -> rows of Kmax
    for (int b = 0; b < B; ++b) std::memcpy(p_pos + sizeof(int) * (size_t)b * (size_t)Kmax, positions_in + (size_t)b * (size_t)pos_ld, sizeof(int) * (size_t)Kmax);
    HIPCHECK(hipMemcpyAsync(d_pos, p_pos, pos_b, hipMemcpyHostToDevice, s));
  }
  // ---- 1 the periods, 2 the positions
  if (run_pitch) {
    PitchArgs a;
    std::memset(&a, 0, sizeof(a));
    wc.in.bind(a);
    a.f0 = d_f0;
    a.ld = (long long)f0_ldw;
    pitch_enqueue(ctx, w, s, pp, a, in_i16 != nullptr, B, Ftotal);
  }
  if (!positions_in) {
    ShiftMarkArgs a;
    std::memset(&a, 0, sizeof(a));
    a.samples = wc.in.d_samples;
    a.f0 = d_f0;
    a.f0_bs = (long long)f0_ldw;
    a.hop_p = pp.hop;
    a.sample_rate = (float)pp.sample_rate;
    a.up = sm->p.up;
    a.down = sm->p.down;
    a.Hs = sm->p.window / 2;
    a.pos = d_pos;
    a.pos_bs = a.pos_ld = (long long)pos_ldw;
    ProfScope ps(ctx, w, KC_SMALL, 4.0 * (double)(Ltotal / a.Hs + 2 * B));
    ps.kernel(KN_SHIFT_MARK);
    hipLaunchKernelGGL(shift_mark_kernel, dim3(B), dim3(64), 0, s, a);
  }
  // ---- 3 the overlap-add: into the workspace for the resampler (PITCH), or out as the resampler's rows go (TEMPO)
  ShiftOlaArgs o;
  std::memset(&o, 0, sizeof(o));
  wc.in.bind(o);
  o.win = sm->win;
  o.up = sm->p.up;
  o.down = sm->p.down;
  o.Hs = sm->p.window / 2;
  o.pos = d_pos;
  o.pos_bs = (long long)pos_ldw;
  if (pitch_mode) {
    o.y = (float*)(base + o_ys);
    o.y_bs = o.y_ld = (long long)Lld;
  } else {
    wave_out_bind(o, wc, plan, tk);
  }
  {
    const long long span = std::max(std::max(o.y ? o.y_ld : 0LL, o.pcm ? o.pcm_ld : 0LL), Lmax);
    const dim3 grid((unsigned)((span + SH_TILE - 1) / SH_TILE), B);
    ProfScope ps(ctx, w, KC_SMALL, 3.0 * (double)Ltotal);
    ps.kernel(KN_SHIFT_OLA);
    if (in_i16) hipLaunchKernelGGL((shift_ola_kernel<true>), grid, dim3(SH_THREADS), 0, s, o);
    else hipLaunchKernelGGL((shift_ola_kernel<false>), grid, dim3(SH_THREADS), 0, s, o);
  }
  // ---- 4 the delivery
  if (pitch_mode) {
    ResampleArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in_f32 = o.y;
    a.in_bs = o.y_bs;
    a.samples = d_L;
    a.out_n = wc.in.d_samples;  // of ceil(L down / up) >= n outputs, the first n
    wave_out_bind(a, wc, plan, tk);
    resample_launch(ctx, w, s, sm->resampler.get(), a, false, Omax, Ototal, B);
    if (normalize) resample_pcm_launch(ctx, w, s, a, wc, B);
  } else if (normalize) {
    resample_pcm_launch(ctx, w, s, o, wc, B, o.up, o.down, d_L);
  }
  if (positions_out && !out_dev) HIPCHECK(hipMemcpyAsync(p_pos, d_pos, pos_b, hipMemcpyDeviceToHost, s));
  if (f0_host) HIPCHECK(hipMemcpyAsync(p_f0, d_f0, f0_b, hipMemcpyDeviceToHost, s));
  CHECK(wc.end());
  // staging rows -> the caller's rows, zeros up to their stride (the kernels wrote the zeros behind a row's own entries)
  auto scatter = [&](void* out, const char* src, size_t have, size_t ld) {
    for (int b = 0; b < B; ++b) {
      char* row = (char*)out + 4 * (size_t)b * ld;
      if (src) std::memcpy(row, src + 4 * (size_t)b * have, 4 * have);
      std::memset(row + 4 * (src ? have : 0), 0, 4 * (ld - (src ? have : 0)));
    }
  };
  if (positions_out && !out_dev) scatter(positions_out, p_pos, (size_t)Kmax, (size_t)pos_ld);
  if (f0_out && !out_dev) scatter(f0_out, f0_host ? p_f0 : nullptr, (size_t)Fmax, (size_t)f0_ld);
  return 0;
}
