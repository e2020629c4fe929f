// mi355tts host runtime — mel analysis: the load and inference entry points (kernel: mel_analysis.h)
// (one translation unit: included once by mi355tts.hip, after griffin_lim_forward.h for the table it shares; the call frame, the
// model table, context_table and the waveform intake: host_call.h)
#pragma once

// frames of a row of N samples (mel_analysis.h)
static int analysis_frames(int framing, long long N) {
  if (framing == MI355TTS_FRAMING_HIFIGAN) return N > MA_PAD ? (int)(N / GL_HOP) : 0;
  return N > GL_FFT ? (int)((N - GL_FFT + GL_HOP - 1) / GL_HOP) : 0;
}

extern "C" int mi355tts_load_analysis(mi355tts_ctx* ctx, const mi355tts_analysis_params* params, const float* mel_basis,
                                      int* model_out) {
  if (!ctx || !params || !mel_basis || !model_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  if (params->num_mels < 1 || params->num_mels > GL_MAX_MELS) return fail(MI355TTS_ERR_INVALID, "num_mels %d outside [1, %d]", params->num_mels, GL_MAX_MELS);
  if (params->framing != MI355TTS_FRAMING_HIFIGAN && params->framing != MI355TTS_FRAMING_REFERENCE)
    return fail(MI355TTS_ERR_INVALID, "unknown framing %d", params->framing);
  if (!(params->mag_eps >= 0.f) || !std::isfinite(params->mag_eps)) return fail(MI355TTS_ERR_INVALID, "mag_eps must be finite and >= 0");
  HIPCHECK(hipSetDevice(ctx->device));
  CHECK(ensure_gl_table(ctx));
  CHECK(context_table(ctx, &ctx->hann_periodic, "analysis window", [](std::vector<float>& win) {
    win.resize(GL_FFT);  // double precision, rounded once, like gl_build_table
    for (int i = 0; i < GL_FFT; ++i) win[i] = (float)(0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * i / GL_FFT));
  }));
  const int M = params->num_mels;
  std::vector<int2> band(M);
  for (int m = 0; m < M; ++m) {
    int k0 = GL_BINS, k1 = 0;
    for (int k = 0; k < GL_BINS; ++k)
      if (mel_basis[(size_t)m * GL_BINS + k] != 0.f) {
        k0 = std::min(k0, k);
        k1 = k + 1;
      }
    band[m] = k1 ? make_int2(k0, k1) : make_int2(0, 0);
  }
  auto am = std::make_shared<AnalysisModel>();
  am->p = *params;
  am->device = ctx->device;
  const size_t n = (size_t)M * GL_BINS;
  if (hipMalloc(&am->basis, n * sizeof(float)) != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc mel basis");
  if (hipMalloc(&am->band, M * sizeof(int2)) != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc mel bands");
  HIPCHECK(hipMemcpy(am->basis, mel_basis, n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(am->band, band.data(), M * sizeof(int2), hipMemcpyHostToDevice));
  return register_model(ctx, std::move(am), model_out);
}

extern "C" int mi355tts_mel_from_audio(mi355tts_ctx* ctx, int model, const float* wav_f32, const int16_t* wav_i16, const int64_t* samples,
                                       int B, int64_t wav_ld, const mi355tts_audio_settings* audio, uint32_t flags, mi355tts_mel** out) {
  if (!ctx || !samples || !out) return fail(MI355TTS_ERR_INVALID, "null argument");
  if ((wav_f32 != nullptr) == (wav_i16 != nullptr)) return fail(MI355TTS_ERR_INVALID, "exactly one of wav_f32 / wav_i16 must be given");
  if (B <= 0 || wav_ld < 0) return fail(MI355TTS_ERR_INVALID, "empty batch or negative wav_ld");
  std::shared_ptr<AnalysisModel> pin;
  CHECK(find_model(ctx, model, &pin));
  const AnalysisModel* am = pin.get();
  const int M = am->p.num_mels;
  WaveIn in{wav_f32, wav_i16, samples, B, wav_ld, (flags & MI355TTS_IN_DEVICE) != 0};
  CHECK(in.check("wav_ld", 30));
  int Fmax = 0;
  long long total = 0;
  std::vector<int32_t> F(B);
  for (int b = 0; b < B; ++b) {
    F[b] = analysis_frames(am->p.framing, samples[b]);
    Fmax = std::max(Fmax, F[b]);
    total += F[b];
  }
  CallFrame f(ctx);
  CHECK(f.open());
  Worker* w = f.w;
  hipStream_t s = f.s;
  const int ld = (Fmax + 3) & ~3;
  CHECK(mel_alloc(ctx, B, M, ld, &f.mel));
  mi355tts_mel* m = f.mel;
  m->max_frames = Fmax;
  m->frames = F;
  CHECK(f.pinned_ints((size_t)2 * B));
  Carver cv;
  in.carve(cv);
  if (Fmax > 0) CHECK(f.reserve(cv.pos, in.bytes));
  for (int b = 0; b < B; ++b) w->pinned[b] = F[b];
  HIPCHECK(hipMemcpyAsync(m->frames_dev, w->pinned, sizeof(int) * B, hipMemcpyHostToDevice, s));
  if (Fmax > 0) {
    CHECK(in.upload(f, w->pinned + B));
    MelAnalysisArgs a;
    std::memset(&a, 0, sizeof(a));
    a.wav_f32 = wav_f32 ? (const float*)in.d : nullptr;
    a.wav_i16 = wav_i16 ? (const short*)in.d : nullptr;
    a.wav_bs = in.bs;
    a.samples = in.d_samples;
    a.frames = m->frames_dev;
    a.reflect = am->p.framing == MI355TTS_FRAMING_HIFIGAN;
    a.window = a.reflect ? ctx->hann_periodic : ctx->gl_table;
    a.tw = reinterpret_cast<const float2*>(ctx->gl_table + GL_FFT);
    a.basis = am->basis;
    a.band = am->band;
    a.raw = m->raw;
    a.voc = m->voc;
    a.M = M;
    a.ld = ld;
    a.mag_eps = am->p.mag_eps;
    a.mt = to_mt(audio);
    a.plain = audio ? 0 : 1;
    // the transform (5 N log2 N of the 512-point complex one + the unpack) and the filter bank's two triangles per bin
    ProfScope ps(ctx, w, KC_SMALL, (double)total * (5.0 * GL_HALF * 9 + 10.0 * GL_HALF + 4.0 * GL_BINS));
    ps.kernel(KN_MEL_ANALYSIS);
    hipLaunchKernelGGL(mel_analysis_kernel, dim3(ld / MA_FRAMES, B), dim3(64 * MA_FRAMES), 0, s, a);
  }
  CHECK(f.finish());
  *out = f.take_mel();
  return 0;
}

extern "C" int mi355tts_mel_plane(const mi355tts_mel* mel, int which, const float** device_ptr, int* ld) {
  if (!mel || !device_ptr || !ld) return fail(MI355TTS_ERR_INVALID, "null argument");
  if (which != 0 && which != 1) return fail(MI355TTS_ERR_INVALID, "which must be 0 (raw) or 1 (vocoder input)");
  *device_ptr = which == 0 ? mel->raw : mel->voc;
  *ld = mel->ld;
  return 0;
}
