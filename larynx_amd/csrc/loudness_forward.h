// mi355tts host runtime — loudness: the load and call entry points (kernels: loudness.h)
// (one translation unit: included once by mi355tts.hip, after resample_forward.h; the call frame, the model table and the
// waveform intake: host_call.h; the row delivery: hifigan_forward.h)
#pragma once

constexpr int LD_MAX_SAMPLES_LOG2 = 24;

// c = a * b, 4 x 4 row-major
static void loudness_matmul(const double* a, const double* b, double* c) {
  double t[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
      t[4 * i + j] = s;
    }
  std::memcpy(c, t, sizeof(t));
}

// pw[k] = M^k for k = 0 .. 256, M = A^LD_CHUNK: A takes (y1[n-1], y1[n-2], y2[n-1], y2[n-2]) one sample on with no input
static void loudness_powers(const mi355tts_loudness_params& p, std::vector<double>& pw) {
  const double sa0 = p.shelf_a[0], sa1 = p.shelf_a[1], hb0 = p.hp_b[0], hb1 = p.hp_b[1], hb2 = p.hp_b[2], ha0 = p.hp_a[0], ha1 = p.hp_a[1];
  const double A[16] = {-sa0, -sa1, 0, 0, 1, 0, 0, 0, hb1 - hb0 * sa0, hb2 - hb0 * sa1, -ha0, -ha1, 0, 0, 1, 0};
  double M[16];
  std::memcpy(M, A, sizeof(M));
  for (int i = 1; i < LD_CHUNK; i *= 2) loudness_matmul(M, M, M);  // (LD_CHUNK is a power of two)
  static_assert((LD_CHUNK & (LD_CHUNK - 1)) == 0, "A^LD_CHUNK by squaring");
  pw.assign((size_t)(LD_THREADS + 1) * 16, 0.0);
  for (int i = 0; i < 4; ++i) pw[5 * i] = 1.0;
  for (int k = 1; k <= LD_THREADS; ++k) loudness_matmul(&pw[(size_t)(k - 1) * 16], M, &pw[(size_t)k * 16]);
}

extern "C" int mi355tts_load_loudness(mi355tts_ctx* ctx, const mi355tts_loudness_params* params, int* model_out) {
  if (!ctx || !params || !model_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  const float* c = params->shelf_b;  // the ten floats lie back to back
  static_assert(offsetof(mi355tts_loudness_params, block) == 10 * sizeof(float), "ten coefficients, then block and hop");
  for (int i = 0; i < 10; ++i)
    if (!std::isfinite(c[i])) return fail(MI355TTS_ERR_INVALID, "coefficient %d is not finite", i);
  if (params->block < 1) return fail(MI355TTS_ERR_INVALID, "block %d < 1", params->block);
  if (params->hop < 1 || params->hop > params->block) return fail(MI355TTS_ERR_INVALID, "hop %d outside [1, block = %d]", params->hop, params->block);
  auto lm = std::make_shared<LoudnessModel>();
  lm->p = *params;
  lm->device = ctx->device;
  std::vector<double> pw;
  loudness_powers(*params, pw);
  HIPCHECK(hipSetDevice(ctx->device));
  if (hipMalloc(&lm->pw, pw.size() * sizeof(double)) != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc loudness table");
  HIPCHECK(hipMemcpy(lm->pw, pw.data(), pw.size() * sizeof(double), hipMemcpyHostToDevice));
  return register_model(ctx, std::move(lm), model_out);
}

extern "C" int mi355tts_loudness(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                                 int64_t in_ld, float target_lufs, float peak_ceiling, float max_gain_db, float* out_f32, int16_t* out_i16,
                                 int64_t out_ld, float* lufs_out, float* gain_out, float* peak_out, float* weighted_out, uint32_t flags) {
  if (!ctx || !samples) return fail(MI355TTS_ERR_INVALID, "null argument");
  if ((in_f32 != nullptr) == (in_i16 != nullptr)) return fail(MI355TTS_ERR_INVALID, "exactly one of in_f32 / in_i16 must be given");
  if (B <= 0 || in_ld < 0) return fail(MI355TTS_ERR_INVALID, "empty batch or negative in_ld");
  if (!(peak_ceiling > 0.f && peak_ceiling <= 1.f)) return fail(MI355TTS_ERR_INVALID, "peak_ceiling %g outside (0, 1]", (double)peak_ceiling);
  if (!std::isfinite(max_gain_db)) return fail(MI355TTS_ERR_INVALID, "max_gain_db is not finite");
  std::shared_ptr<LoudnessModel> pin;
  CHECK(find_model(ctx, model, &pin));
  const LoudnessModel* lm = pin.get();
  WaveIn in{in_f32, in_i16, samples, B, in_ld, (flags & MI355TTS_IN_DEVICE) != 0};
  CHECK(in.check("in_ld", LD_MAX_SAMPLES_LOG2));
  const long long Nmax = in.Nmax;
  const bool any_out = out_f32 || out_i16;
  if (any_out && out_ld < Nmax) return fail(MI355TTS_ERR_INVALID, "out_ld %lld < %lld samples of the longest row", (long long)out_ld, Nmax);
  const bool out_dev = (flags & MI355TTS_OUT_DEVICE) != 0;
  CallFrame f(ctx);
  CHECK(f.open());
  Worker* w = f.w;
  hipStream_t s = f.s;
  const OutRows rows = {nullptr, nullptr, 0, {out_f32, out_i16, out_ld, 0, 0, (size_t)Nmax}};
  if (Nmax == 0) {  // nothing to measure in any row: -inf, gain 1, every output zero
    for (int b = 0; b < B; ++b) {
      if (lufs_out) lufs_out[b] = -INFINITY;
      if (gain_out) gain_out[b] = 1.f;
      if (peak_out) peak_out[b] = 0.f;
    }
    if (weighted_out) CHECK((RowWriter{out_dev, s}).zero(weighted_out, (size_t)B * (size_t)in_ld));
    return zero_outputs(f, rows, B, out_dev);
  }
  CHECK(f.pinned_ints(B));
  const int block = lm->p.block, hop = lm->p.hop;
  const size_t Nld = (size_t)((Nmax + 7) & ~7LL);
  const int gmax = (int)((Nmax + LD_GROUP - 1) / LD_GROUP);
  const long long smax = (Nmax + hop - 1) / hop;
  const long long zmax = Nmax >= block ? (Nmax - block) / hop + 1 : 1;
  const bool w_direct = weighted_out && out_dev;
  Carver cv;
  in.carve(cv);
  const size_t o_cs = cv.take(sizeof(double) * 4 * (size_t)B * gmax * LD_THREADS);
  const size_t o_gs = cv.take(sizeof(double) * 4 * (size_t)B * gmax);
  const size_t o_gp = cv.take(sizeof(float) * (size_t)B * gmax);
  const size_t o_w = cv.take(w_direct ? 0 : sizeof(float) * (size_t)B * Nld);
  const size_t o_seg = cv.take(sizeof(double) * 2 * (size_t)B * smax);
  const size_t o_z = cv.take(sizeof(float) * (size_t)B * zmax);
  const size_t o_res = cv.take(sizeof(float) * 3 * (size_t)B);
  const size_t o_y = cv.take(out_f32 && !out_dev ? sizeof(float) * (size_t)B * Nld : 0);
  const size_t o_pcm = cv.take(out_i16 && !out_dev ? sizeof(short) * (size_t)B * Nld : 0);
  // host outputs wait in the pinned staging behind the staged input: the delivered rows and the per-row results, then the
  // K-weighted rows
  const Staging st = host_staging(B, out_f32 && !out_dev, Nld, out_i16 && !out_dev, Nld, in.bytes, sizeof(float) * 3 * (size_t)B);
  const size_t w_host = weighted_out && !out_dev ? sizeof(float) * (size_t)B * Nld : 0;
  CHECK(f.reserve(cv.pos, st.end() + w_host));
  char* base = w->arena;
  CHECK(in.upload(f, w->pinned));
  LoudnessArgs a;
  std::memset(&a, 0, sizeof(a));
  a.in_f32 = in_f32 ? (const float*)in.d : nullptr;
  a.in_i16 = in_i16 ? (const short*)in.d : nullptr;
  a.in_bs = in.bs;
  a.samples = in.d_samples;
  for (int i = 0; i < 3; ++i) {
    a.sb[i] = lm->p.shelf_b[i];
    a.hb[i] = lm->p.hp_b[i];
  }
  for (int i = 0; i < 2; ++i) {
    a.sa[i] = lm->p.shelf_a[i];
    a.ha[i] = lm->p.hp_a[i];
  }
  a.pw = lm->pw;
  a.block = block;
  a.hop = hop;
  a.abs_thr = std::pow(10.0, (-70.0 + 0.691) / 10.0);
  a.cstate = (double*)(base + o_cs);
  a.gstate = (double*)(base + o_gs);
  a.gpeak = (float*)(base + o_gp);
  a.gmax = gmax;
  a.w = w_direct ? weighted_out : (float*)(base + o_w);
  a.w_bs = a.w_ld = w_direct ? (long long)in_ld : (long long)Nld;
  a.seg = (double*)(base + o_seg);
  a.smax = smax;
  a.z = (float*)(base + o_z);
  a.zmax = zmax;
  a.target = target_lufs;
  a.ceiling = peak_ceiling;
  a.max_gain = std::pow(10.0, (double)max_gain_db / 20.0);
  a.res = (float*)(base + o_res);
  long long total = 0;
  for (int b = 0; b < B; ++b) total += samples[b];
  const dim3 tb(LD_THREADS);
  {
    ProfScope ps(ctx, w, KC_SMALL, 20.0 * (double)total);
    ps.kernel(KN_LOUD_CHUNK);
    if (in_i16) hipLaunchKernelGGL(loudness_chunk_kernel<true>, dim3(gmax, B), tb, 0, s, a);
    else hipLaunchKernelGGL(loudness_chunk_kernel<false>, dim3(gmax, B), tb, 0, s, a);
  }
  {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    ps.kernel(KN_LOUD_CARRY);
    hipLaunchKernelGGL(loudness_carry_kernel, dim3(B), tb, 0, s, a);
  }
  {
    // (the grid also covers the zero tail of a row the caller's device buffer holds: up to its stride)
    const unsigned gx = (unsigned)((std::max(Nmax, a.w_ld) + LD_GROUP - 1) / LD_GROUP);
    ProfScope ps(ctx, w, KC_SMALL, 20.0 * (double)total);
    ps.kernel(KN_LOUD_WEIGHT);
    if (in_i16) hipLaunchKernelGGL(loudness_weight_kernel<true>, dim3(gx, B), tb, 0, s, a);
    else hipLaunchKernelGGL(loudness_weight_kernel<false>, dim3(gx, B), tb, 0, s, a);
  }
  {
    ProfScope ps(ctx, w, KC_SMALL, 2.0 * (double)total);
    ps.kernel(KN_LOUD_SEGMENT);
    hipLaunchKernelGGL(loudness_segment_kernel, dim3((unsigned)smax, B), tb, 0, s, a);
  }
  {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    ps.kernel(KN_LOUD_GATE);
    hipLaunchKernelGGL(loudness_gate_kernel, dim3(B), tb, 0, s, a);
  }
  float* const d_y = !out_f32 ? nullptr : out_dev ? out_f32 : (float*)(base + o_y);
  short* const d_pcm = !out_i16 ? nullptr : out_dev ? (short*)out_i16 : (short*)(base + o_pcm);
  if (any_out) {
    const long long ld = out_dev ? (long long)out_ld : (long long)Nld;
    const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((ld + 1023) / 1024, 1), 256);
    ProfScope ps(ctx, w, KC_SMALL, (double)total);
    ps.kernel(KN_LOUD_APPLY);
    if (in_i16) hipLaunchKernelGGL(loudness_apply_kernel<true>, dim3(gx, B), dim3(256), 0, s, a, d_y, d_pcm, ld, ld);
    else hipLaunchKernelGGL(loudness_apply_kernel<false>, dim3(gx, B), dim3(256), 0, s, a, d_y, d_pcm, ld, ld);
  }
  char* const pw_host = w->pinned_out + st.end();
  if (w_host) HIPCHECK(hipMemcpyAsync(pw_host, a.w, w_host, hipMemcpyDeviceToHost, s));
  std::vector<float> res((size_t)3 * B);
  // (with device outputs the staging holds no rows: the per-row results alone travel, and scatter_rows finds nothing to write)
  const OutRows host_rows = out_dev ? OutRows{nullptr, nullptr, 0, {nullptr, nullptr, 0, 0, 0, 0}} : rows;
  CHECK(deliver_rows(f, host_rows, B, WavRows{d_y, Nld, d_pcm, Nld}, st, true, res.data(), a.res));
  for (int b = 0; b < B; ++b) {
    if (lufs_out) lufs_out[b] = res[3 * b];
    if (gain_out) gain_out[b] = res[3 * b + 1];
    if (peak_out) peak_out[b] = res[3 * b + 2];
    if (w_host) {
      float* dst = weighted_out + (size_t)b * (size_t)in_ld;
      std::memcpy(dst, pw_host + sizeof(float) * (size_t)b * Nld, sizeof(float) * (size_t)samples[b]);
      std::memset(dst + samples[b], 0, sizeof(float) * ((size_t)in_ld - (size_t)samples[b]));
    }
  }
  return 0;
}
