// mi355tts host runtime — mel analysis: the load and inference entry points (kernel: mel_analysis.h)
// (one translation unit: included once by mi355tts.hip, after griffin_lim_forward.h for the table it shares)
#pragma once

static int find_analysis(mi355tts_ctx* ctx, int model, std::shared_ptr<AnalysisModel>* out) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  auto it = ctx->analysis.find(model);
  if (it == ctx->analysis.end()) return fail(MI355TTS_ERR_NO_MODEL, "no analysis model %d", model);
  *out = it->second;
  return 0;
}

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
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->hann_periodic) {  // double precision, rounded once, like gl_build_table
      std::vector<float> win(GL_FFT);
      for (int i = 0; i < GL_FFT; ++i) win[i] = (float)(0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * i / GL_FFT));
      float* d = nullptr;
      if (hipMalloc(&d, win.size() * sizeof(float)) != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc analysis window");
      if (hipMemcpy(d, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d);
        return fail(MI355TTS_ERR_HIP, "analysis window upload failed");
      }
      ctx->hann_periodic = d;
    }
  }
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
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int id = ctx->next_id++;
  ctx->analysis[id] = std::move(am);
  *model_out = id;
  return 0;
}

extern "C" int mi355tts_mel_from_audio(mi355tts_ctx* ctx, int model, const float* wav_f32, const int16_t* wav_i16, const int64_t* samples,
                                       int B, int64_t wav_ld, const mi355tts_audio_settings* audio, uint32_t flags, mi355tts_mel** out) {
  if (!ctx || !samples || !out) return fail(MI355TTS_ERR_INVALID, "null argument");
  if ((wav_f32 != nullptr) == (wav_i16 != nullptr)) return fail(MI355TTS_ERR_INVALID, "exactly one of wav_f32 / wav_i16 must be given");
  if (B <= 0 || wav_ld < 0) return fail(MI355TTS_ERR_INVALID, "empty batch or negative wav_ld");
  std::shared_ptr<AnalysisModel> pin;
  CHECK(find_analysis(ctx, model, &pin));
  const AnalysisModel* am = pin.get();
  const int M = am->p.num_mels;
  int Fmax = 0;
  long long Nmax = 0, total = 0;
  std::vector<int32_t> F(B);
  for (int b = 0; b < B; ++b) {
    if (samples[b] < 0 || samples[b] > wav_ld)
      return fail(MI355TTS_ERR_INVALID, "samples[%d]=%lld outside [0, wav_ld=%lld]", b, (long long)samples[b], (long long)wav_ld);
    if (samples[b] > (1LL << 30)) return fail(MI355TTS_ERR_INVALID, "samples[%d]=%lld > 2^30", b, (long long)samples[b]);
    F[b] = analysis_frames(am->p.framing, samples[b]);
    Fmax = std::max(Fmax, F[b]);
    Nmax = std::max(Nmax, (long long)samples[b]);
    total += F[b];
  }
  const bool in_dev = (flags & MI355TTS_IN_DEVICE) != 0;
  HIPCHECK(hipSetDevice(ctx->device));
  const int ld = (Fmax + 3) & ~3;
  mi355tts_mel* m = nullptr;
  CHECK(mel_alloc(ctx, B, M, ld, &m));
  struct Drop {  // the mel, unless the call succeeds
    mi355tts_mel* m;
    ~Drop() { mel_destroy(m); }
  } drop{m};
  m->max_frames = Fmax;
  m->frames = F;
  Worker* w = nullptr;
  CHECK(acquire_worker(ctx, &w));
  WorkerGuard guard{ctx, w};
  hipStream_t s = w->stream;
  if ((size_t)2 * B > w->pinned_ints) return fail(MI355TTS_ERR_INVALID, "batch too large");
  for (int b = 0; b < B; ++b) {
    w->pinned[b] = F[b];
    w->pinned[B + b] = (int)samples[b];
  }
  HIPCHECK(hipMemcpyAsync(m->frames_dev, w->pinned, sizeof(int) * B, hipMemcpyHostToDevice, s));
  if (Fmax > 0) {
    // a host waveform: the rows' samples -> pinned staging -> the workspace (row stride Nld); a device one is read in place
    const size_t esz = wav_f32 ? sizeof(float) : sizeof(int16_t);
    const size_t Nld = (size_t)((Nmax + 7) & ~7LL);
    Carver cv;
    const size_t o_n = cv.take(sizeof(int) * B);
    const size_t o_wav = cv.take(in_dev ? 0 : esz * (size_t)B * Nld);
    CHECK(reserve(w, cv.pos));
    char* base = w->arena;
    int* d_samples = (int*)(base + o_n);
    HIPCHECK(hipMemcpyAsync(d_samples, w->pinned + B, sizeof(int) * B, hipMemcpyHostToDevice, s));
    const void* d_wav = wav_f32 ? (const void*)wav_f32 : (const void*)wav_i16;
    long long wav_bs = wav_ld;
    if (!in_dev) {
      CHECK(reserve_pinned_out(w, esz * (size_t)B * Nld));
      for (int b = 0; b < B; ++b) {
        char* dst = w->pinned_out + esz * (size_t)b * Nld;
        std::memcpy(dst, (const char*)d_wav + esz * (size_t)b * (size_t)wav_ld, esz * (size_t)samples[b]);
        std::memset(dst + esz * (size_t)samples[b], 0, esz * (Nld - (size_t)samples[b]));
      }
      HIPCHECK(hipMemcpyAsync(base + o_wav, w->pinned_out, esz * (size_t)B * Nld, hipMemcpyHostToDevice, s));
      d_wav = base + o_wav;
      wav_bs = (long long)Nld;
    }
    MelAnalysisArgs a;
    std::memset(&a, 0, sizeof(a));
    a.wav_f32 = wav_f32 ? (const float*)d_wav : nullptr;
    a.wav_i16 = wav_i16 ? (const short*)d_wav : nullptr;
    a.wav_bs = wav_bs;
    a.samples = d_samples;
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
  HIPCHECK(mi355_sync(s));
  HIPCHECK(hipGetLastError());
  drop.m = nullptr;
  *out = m;
  return 0;
}

extern "C" int mi355tts_mel_plane(const mi355tts_mel* mel, int which, const float** device_ptr, int* ld) {
  if (!mel || !device_ptr || !ld) return fail(MI355TTS_ERR_INVALID, "null argument");
  if (which != 0 && which != 1) return fail(MI355TTS_ERR_INVALID, "which must be 0 (raw) or 1 (vocoder input)");
  *device_ptr = which == 0 ? mel->raw : mel->voc;
  *ld = mel->ld;
  return 0;
}
