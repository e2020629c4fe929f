// mi355tts host runtime — the Griffin-Lim vocoder's load and inference entry points (kernels: griffin_lim.h)
// (one translation unit: included once by mi355tts.hip, after hifigan_forward.h; the call frame, the model table and
// context_table: host_call.h; the row delivery: host_rows.h)
#pragma once

// window + twiddles in double precision, rounded once: tab[i] = np.hanning(1024)[i]; then (cos, -sin)(2 pi m / 1024) with the
// multiples of a quarter turn exact
static void gl_build_table(std::vector<float>& t) {
  t.resize(GL_TAB_FLOATS);
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < GL_FFT; ++i) t[i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * i / (GL_FFT - 1)));
  for (int m = 0; m < GL_FFT; ++m) {
    double c = std::cos(2.0 * pi * m / GL_FFT), s = -std::sin(2.0 * pi * m / GL_FFT);
    if (m % (GL_FFT / 4) == 0) {
      c = std::nearbyint(c);
      s = std::nearbyint(s);
    }
    t[GL_FFT + 2 * m] = (float)c;
    t[GL_FFT + 2 * m + 1] = (float)s;
  }
}

// the context's copy of the table
static int ensure_gl_table(mi355tts_ctx* ctx) { return context_table(ctx, &ctx->gl_table, "Griffin-Lim table", gl_build_table); }

extern "C" int mi355tts_load_griffin_lim(mi355tts_ctx* ctx, const mi355tts_griffin_lim_params* params, const float* mel_basis,
                                         int* model_out) {
  if (!ctx || !params || !mel_basis || !model_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  if (params->num_mels < 1 || params->num_mels > GL_MAX_MELS) return fail(MI355TTS_ERR_INVALID, "num_mels %d outside [1, %d]", params->num_mels, GL_MAX_MELS);
  if (params->iterations < 0 || params->iterations > 100000) return fail(MI355TTS_ERR_INVALID, "iterations %d outside [0, 100000]", params->iterations);
  if (!(params->mel_scaling > 0.f) || !std::isfinite(params->mel_scaling)) return fail(MI355TTS_ERR_INVALID, "mel_scaling must be positive");
  HIPCHECK(hipSetDevice(ctx->device));
  CHECK(ensure_gl_table(ctx));
  auto gm = std::make_shared<GriffinLimModel>();
  gm->p = *params;
  gm->device = ctx->device;
  const size_t n = (size_t)params->num_mels * GL_BINS;
  if (hipMalloc(&gm->basis, n * sizeof(float)) != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc mel basis");
  HIPCHECK(hipMemcpy(gm->basis, mel_basis, n * sizeof(float), hipMemcpyHostToDevice));
  return register_model(ctx, std::move(gm), model_out);
}

extern "C" int mi355tts_griffin_lim_infer(mi355tts_ctx* ctx, int model, const mi355tts_mel* mel, const float* phase0, uint64_t seed,
                                          float* phase_out, float* wav_f32, int16_t* wav_i16, int64_t wav_ld, int iterations,
                                          uint32_t flags) {
  if (!ctx || !mel) return fail(MI355TTS_ERR_INVALID, "null argument");
  std::shared_ptr<GriffinLimModel> pin;
  CHECK(find_model(ctx, model, &pin));
  const GriffinLimModel* gm = pin.get();
  if (mel->ctx != ctx) return fail(MI355TTS_ERR_INVALID, "mel belongs to another context");
  if (mel->M != gm->p.num_mels) return fail(MI355TTS_ERR_INVALID, "mel has %d channels, the vocoder expects %d", mel->M, gm->p.num_mels);
  const int iters = iterations > 0 ? iterations : gm->p.iterations;
  if (iters > 100000) return fail(MI355TTS_ERR_INVALID, "iterations %d > 100000", iters);
  const int B = mel->B;
  const int T = std::max(mel->max_frames - 1, 0);  // STFT frames of the longest row
  const long long N = T > 0 ? (long long)T * GL_HOP + GL_FFT : 0;
  if ((wav_f32 || wav_i16) && wav_ld < N) return fail(MI355TTS_ERR_TOO_SMALL, "wav_ld %lld < %lld samples", (long long)wav_ld, N);
  if (wav_ld < 0) return fail(MI355TTS_ERR_INVALID, "negative wav_ld");
  const bool in_dev = (flags & MI355TTS_IN_DEVICE) != 0, out_dev = (flags & MI355TTS_OUT_DEVICE) != 0;
  CallFrame f(ctx);
  CHECK(f.open());
  Worker* w = f.w;
  hipStream_t s = f.s;
  const OutRows rows = {nullptr, nullptr, 0, {wav_f32, wav_i16, wav_ld, 0, 0, (size_t)N}};
  if (T == 0) return zero_outputs(f, rows, B, out_dev);  // every row has fewer than 2 frames: empty signals
  const size_t nph = (size_t)B * GL_BINS * T;
  const size_t Nld = (size_t)((N + 3) & ~3LL);
  Carver cv;
  const size_t o_mag = cv.take(sizeof(float) * (size_t)B * T * GL_MAG_LD);
  const size_t o_f0 = cv.take(sizeof(float) * (size_t)B * T * GL_FFT);
  const size_t o_f1 = cv.take(sizeof(float) * (size_t)B * T * GL_FFT);
  const size_t o_wav = cv.take(sizeof(float) * (size_t)B * Nld);
  const size_t o_i16 = cv.take(sizeof(short) * (size_t)B * Nld);
  const size_t o_peak = cv.take(sizeof(unsigned) * (size_t)B);
  const size_t o_pin = cv.take(phase0 && !in_dev ? sizeof(float) * nph : 0);
  const size_t o_pout = cv.take(phase_out && !out_dev ? sizeof(float) * nph : 0);
  // host outputs wait in the pinned staging: the float rows, the int16 rows, the phases
  const Staging st = host_staging(B, wav_f32 && !out_dev, Nld, wav_i16 && !out_dev, Nld, 0, phase_out && !out_dev ? sizeof(float) * nph : 0);
  CHECK(f.reserve(cv.pos, st.end()));
  char* base = w->arena;
  float* mag = (float*)(base + o_mag);
  float* fb[2] = {(float*)(base + o_f0), (float*)(base + o_f1)};
  unsigned* peak = (unsigned*)(base + o_peak);
  const float* dph_in = phase0;
  if (phase0 && !in_dev) {
    HIPCHECK(hipMemcpyAsync(base + o_pin, phase0, sizeof(float) * nph, hipMemcpyHostToDevice, s));
    dph_in = (const float*)(base + o_pin);
  }
  float* dph_out = phase_out ? (out_dev ? phase_out : (float*)(base + o_pout)) : nullptr;
  if (dph_out) HIPCHECK(hipMemsetAsync(dph_out, 0, sizeof(float) * nph, s));  // (frames past a short row's own stay zero)
  const int* d_frames = mel->frames_dev;
  const float* tab = ctx->gl_table;
  {
    ProfScope ps(ctx, w, KC_SMALL, 2.0 * gm->p.num_mels * GL_BINS * (double)T * B);
    ps.kernel(KN_GL_MAG);
    hipLaunchKernelGGL(griffin_lim_mag_kernel, dim3((T + GL_MAG_FRAMES - 1) / GL_MAG_FRAMES, B), dim3(256), 0, s, mel->voc,
                       (long long)mel->M * mel->ld, mel->ld, d_frames, mel->M, gm->basis, gm->p.mel_scaling, mag, T);
  }
  {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    ps.kernel(KN_GL_INIT);
    hipLaunchKernelGGL(griffin_lim_init_kernel, dim3(T, B), dim3(64), 0, s, mag, d_frames, T, dph_in, dph_out, T, seed, tab, fb[0]);
  }
  int cur = 0;
  for (int it = 0; it < iters; ++it) {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    ps.kernel(KN_GL_ITER);
    hipLaunchKernelGGL(griffin_lim_iter_kernel, dim3(T, B), dim3(64), 0, s, fb[cur], fb[cur ^ 1], mag, d_frames, T, tab);
    cur ^= 1;
  }
  // the float rows: straight into the caller's device buffer, or into the workspace the host copy (and the int16 pass) reads
  float* wav = (float*)(base + o_wav);
  long long wbs = (long long)Nld, wld = (long long)Nld;
  if (out_dev && wav_f32) {
    wav = wav_f32;
    wbs = wld = wav_ld;
  }
  if (wav_f32 || wav_i16) {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    if (wav_i16) HIPCHECK(hipMemsetAsync(peak, 0, sizeof(unsigned) * B, s));
    ps.kernel(KN_GL_OUT);
    hipLaunchKernelGGL(griffin_lim_out_kernel, dim3(128, B), dim3(256), 0, s, fb[cur], T, d_frames, wav, wbs, wld, wav_i16 ? peak : (unsigned*)nullptr);
  }
  short* i16 = (short*)(base + o_i16);
  if (wav_i16) {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    ps.kernel(KN_GL_INT16);
    if (out_dev) hipLaunchKernelGGL(griffin_lim_int16_kernel, dim3(128, B), dim3(256), 0, s, wav, wbs, d_frames, peak, wav_i16, (long long)wav_ld, (long long)wav_ld);
    else hipLaunchKernelGGL(griffin_lim_int16_kernel, dim3(128, B), dim3(256), 0, s, wav, wbs, d_frames, peak, i16, (long long)Nld, (long long)Nld);
  }
  return out_dev ? f.finish() : deliver_rows(f, rows, B, WavRows{wav, Nld, i16, Nld}, st, true, phase_out, dph_out);
}
