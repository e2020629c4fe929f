// mi355tts host runtime — loudness: the load and call entry points (kernels: loudness.h)
// (one translation unit: included once by mi355tts.hip, after resample_forward.h; the model table and upload: host_call.h; the
// frame of the call, WaveCall, and the row delivery: host_rows.h)
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
  CHECK(upload(&lm->pw, pw, "loudness table"));
  return register_model(ctx, std::move(lm), model_out);
}

extern "C" int mi355tts_loudness(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                                 int64_t in_ld, float target_lufs, float peak_ceiling, float max_gain_db, float* out_f32, int16_t* out_i16,
                                 int64_t out_ld, float* lufs_out, float* gain_out, float* peak_out, float* weighted_out, uint32_t flags) {
  WaveCall wc(ctx, in_f32, in_i16, samples, B, in_ld, out_f32, out_i16, out_ld, flags);
  CHECK(wc.check_args());
  if (!(peak_ceiling > 0.f && peak_ceiling <= 1.f)) return fail(MI355TTS_ERR_INVALID, "peak_ceiling %g outside (0, 1]", (double)peak_ceiling);
  if (!std::isfinite(max_gain_db)) return fail(MI355TTS_ERR_INVALID, "max_gain_db is not finite");
  std::shared_ptr<LoudnessModel> pin;
  CHECK(find_model(ctx, model, &pin));
  const LoudnessModel* lm = pin.get();
  CHECK(wc.in.check("in_ld", LD_MAX_SAMPLES_LOG2));
  const long long Nmax = wc.in.Nmax;
  CHECK(wc.check_out(Nmax));
  CHECK(wc.open(weighted_out, {lufs_out, gain_out, peak_out}));  // the side plane: the K-weighted rows
  Worker* w = wc.f.w;
  hipStream_t s = wc.f.s;
  if (Nmax == 0) return wc.empty({-INFINITY, 1.f, 0.f});  // nothing to measure in any row: -inf, gain 1, peak 0
  CHECK(wc.f.pinned_ints(B));
  const int block = lm->p.block, hop = lm->p.hop;
  const int gmax = (int)((Nmax + LD_GROUP - 1) / LD_GROUP);
  const long long smax = (Nmax + hop - 1) / hop;
  const long long zmax = Nmax >= block ? (Nmax - block) / hop + 1 : 1;
  Carver cv = wc.carve();
  const size_t o_cs = cv.take(sizeof(double) * 4 * (size_t)B * gmax * LD_THREADS);
  const size_t o_gs = cv.take(sizeof(double) * 4 * (size_t)B * gmax);
  const size_t o_gp = cv.take(sizeof(float) * (size_t)B * gmax);
  const size_t o_w = cv.take(weighted_out ? 0 : sizeof(float) * (size_t)B * wc.in.Nld);  // the weighted rows nobody receives
  const size_t o_seg = cv.take(sizeof(double) * 2 * (size_t)B * smax);
  const size_t o_z = cv.take(sizeof(float) * (size_t)B * zmax);
  CHECK(wc.reserve(cv));
  char* base = w->arena;
  LoudnessArgs a;
  std::memset(&a, 0, sizeof(a));
  wc.in.bind(a);
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
  a.w = weighted_out ? wc.d_side : (float*)(base + o_w);
  a.w_bs = a.w_ld = weighted_out ? wc.side_ld : (long long)wc.in.Nld;
  a.seg = (double*)(base + o_seg);
  a.smax = smax;
  a.z = (float*)(base + o_z);
  a.zmax = zmax;
  a.target = target_lufs;
  a.ceiling = peak_ceiling;
  a.max_gain = std::pow(10.0, (double)max_gain_db / 20.0);
  a.res = wc.d_res;
  const long long total = wc.in.total;
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
  if (out_f32 || out_i16) {
    const long long ld = wc.ld;
    const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((ld + 1023) / 1024, 1), 256);
    ProfScope ps(ctx, w, KC_SMALL, (double)total);
    ps.kernel(KN_LOUD_APPLY);
    if (in_i16) hipLaunchKernelGGL(loudness_apply_kernel<true>, dim3(gx, B), dim3(256), 0, s, a, wc.d_y, wc.d_pcm, ld, ld);
    else hipLaunchKernelGGL(loudness_apply_kernel<false>, dim3(gx, B), dim3(256), 0, s, a, wc.d_y, wc.d_pcm, ld, ld);
  }
  return wc.end();
}
