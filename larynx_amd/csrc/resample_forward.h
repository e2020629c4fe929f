// mi355tts host runtime — resampling: the load, length and call entry points (kernels: resample.h)
// (one translation unit: included once by mi355tts.hip, after hifigan_forward.h for the row delivery it shares)
#pragma once

static int find_resampler(mi355tts_ctx* ctx, int model, std::shared_ptr<ResamplerModel>* out) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  auto it = ctx->resampler.find(model);
  if (it == ctx->resampler.end()) return fail(MI355TTS_ERR_NO_MODEL, "no resampler %d", model);
  *out = it->second;
  return 0;
}

constexpr long long RS_MAX_SAMPLES = 1LL << 24;
static long long resample_len(const ResamplerModel* rm, long long n) { return (n * rm->p.up + rm->p.down - 1) / rm->p.down; }

extern "C" int mi355tts_load_resampler(mi355tts_ctx* ctx, const mi355tts_resampler_params* params, const float* taps, int* model_out) {
  if (!ctx || !params || !taps || !model_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  const int up = params->up, down = params->down;
  if (up < 1 || up > RS_MAX_UD || down < 1 || down > RS_MAX_UD) return fail(MI355TTS_ERR_INVALID, "up %d / down %d outside [1, %d]", up, down, RS_MAX_UD);
  int g = up;
  for (int r = down; r;) {
    const int t = g % r;
    g = r;
    r = t;
  }
  if (g != 1) return fail(MI355TTS_ERR_INVALID, "up %d and down %d are not coprime", up, down);
  if (params->half_len < 0) return fail(MI355TTS_ERR_INVALID, "half_len %d < 0", params->half_len);
  const long long ntaps = 2LL * params->half_len + 1;
  const long long T = (ntaps + up - 1) / up;
  if (T > RS_MAX_T) return fail(MI355TTS_ERR_INVALID, "%lld taps per phase > %d", T, RS_MAX_T);
  for (long long j = 0; j < ntaps; ++j)
    if (!std::isfinite(taps[j])) return fail(MI355TTS_ERR_INVALID, "tap %lld is not finite", j);
  auto rm = std::make_shared<ResamplerModel>();
  rm->p = *params;
  rm->device = ctx->device;
  rm->T = (int)T;
  rm->Tp = ((int)T + 3) & ~3;
  std::vector<float> table((size_t)up * rm->Tp, 0.f);  // [p][t] = taps[p + t * up]
  for (long long j = 0; j < ntaps; ++j) table[(size_t)(j % up) * rm->Tp + (size_t)(j / up)] = taps[j];
  HIPCHECK(hipSetDevice(ctx->device));
  if (hipMalloc(&rm->table, table.size() * sizeof(float)) != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc resampler table");
  HIPCHECK(hipMemcpy(rm->table, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int id = ctx->next_id++;
  ctx->resampler[id] = std::move(rm);
  *model_out = id;
  return 0;
}

extern "C" int64_t mi355tts_resample_length(mi355tts_ctx* ctx, int model, int64_t samples) {
  if (!ctx) return fail(MI355TTS_ERR_INVALID, "null argument");
  std::shared_ptr<ResamplerModel> pin;
  CHECK(find_resampler(ctx, model, &pin));
  if (samples < 0 || samples > RS_MAX_SAMPLES) return fail(MI355TTS_ERR_INVALID, "samples %lld outside [0, 2^24]", (long long)samples);
  return resample_len(pin.get(), samples);
}

extern "C" int mi355tts_resample(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                                 int64_t in_ld, float* out_f32, int16_t* out_i16, int64_t out_ld, int pcm_mode, int64_t* samples_out,
                                 uint32_t flags) {
  if (!ctx || !samples) return fail(MI355TTS_ERR_INVALID, "null argument");
  if ((in_f32 != nullptr) == (in_i16 != nullptr)) return fail(MI355TTS_ERR_INVALID, "exactly one of in_f32 / in_i16 must be given");
  if (!out_f32 && !out_i16) return fail(MI355TTS_ERR_INVALID, "no output: give out_f32, out_i16 or both");
  if (B <= 0 || in_ld < 0) return fail(MI355TTS_ERR_INVALID, "empty batch or negative in_ld");
  if (pcm_mode != MI355TTS_PCM_SATURATE && pcm_mode != MI355TTS_PCM_NORMALIZE) return fail(MI355TTS_ERR_INVALID, "unknown pcm_mode %d", pcm_mode);
  std::shared_ptr<ResamplerModel> pin;
  CHECK(find_resampler(ctx, model, &pin));
  const ResamplerModel* rm = pin.get();
  long long Nmax = 0, Omax = 0, total = 0;
  for (int b = 0; b < B; ++b) {
    if (samples[b] < 0 || samples[b] > in_ld)
      return fail(MI355TTS_ERR_INVALID, "samples[%d]=%lld outside [0, in_ld=%lld]", b, (long long)samples[b], (long long)in_ld);
    if (samples[b] > RS_MAX_SAMPLES) return fail(MI355TTS_ERR_INVALID, "samples[%d]=%lld > 2^24", b, (long long)samples[b]);
    const long long o = resample_len(rm, samples[b]);
    Nmax = std::max(Nmax, (long long)samples[b]);
    Omax = std::max(Omax, o);
    total += o;
  }
  if (out_ld < Omax) return fail(MI355TTS_ERR_INVALID, "out_ld %lld < %lld samples of the longest row", (long long)out_ld, Omax);
  if (samples_out)
    for (int b = 0; b < B; ++b) samples_out[b] = resample_len(rm, samples[b]);
  const bool in_dev = (flags & MI355TTS_IN_DEVICE) != 0, out_dev = (flags & MI355TTS_OUT_DEVICE) != 0;
  const bool normalize = out_i16 && pcm_mode == MI355TTS_PCM_NORMALIZE;
  HIPCHECK(hipSetDevice(ctx->device));
  Worker* w = nullptr;
  CHECK(acquire_worker(ctx, &w));
  WorkerGuard guard{ctx, w};
  hipStream_t s = w->stream;
  const OutRows rows = {nullptr, nullptr, 0, {out_f32, out_i16, out_ld, 0, 0, (size_t)Omax}};
  if (Omax == 0) return zero_outputs(rows, B, RowWriter{out_dev, s});
  if ((size_t)B > w->pinned_ints) return fail(MI355TTS_ERR_INVALID, "batch too large");
  // host rows travel through the workspace at strides Nld (in) and Old (out); device rows are read and written in place
  const size_t esz = in_f32 ? sizeof(float) : sizeof(int16_t);
  const size_t Nld = (size_t)((Nmax + 7) & ~7LL), Old = (size_t)((Omax + 7) & ~7LL);
  const long long tiles = (Omax + RS_TILE - 1) / RS_TILE;
  const bool y_direct = out_dev && out_f32;              // the float rows straight into the caller's device buffer
  const bool y_ws = !y_direct && (out_f32 || normalize);  // or into the workspace: for the host copy, or for the second launch only
  Carver cv;
  const size_t o_n = cv.take(sizeof(int) * B);
  const size_t o_in = cv.take(in_dev ? 0 : esz * (size_t)B * Nld);
  const size_t o_y = cv.take(y_ws ? sizeof(float) * (size_t)B * Old : 0);
  const size_t o_pcm = cv.take(out_i16 && !out_dev ? sizeof(short) * (size_t)B * Old : 0);
  const size_t o_peak = cv.take(normalize ? sizeof(float) * (size_t)B * tiles : 0);
  CHECK(reserve(w, cv.pos));
  const size_t in_b = in_dev ? 0 : esz * (size_t)B * Nld;
  const size_t f32_b = out_f32 && !out_dev ? sizeof(float) * (size_t)B * Old : 0;
  const size_t i16_b = out_i16 && !out_dev ? sizeof(short) * (size_t)B * Old : 0;
  CHECK(reserve_pinned_out(w, in_b + f32_b + i16_b));
  char* base = w->arena;
  int* d_samples = (int*)(base + o_n);
  for (int b = 0; b < B; ++b) w->pinned[b] = (int)samples[b];
  HIPCHECK(hipMemcpyAsync(d_samples, w->pinned, sizeof(int) * B, hipMemcpyHostToDevice, s));
  const void* d_in = in_f32 ? (const void*)in_f32 : (const void*)in_i16;
  long long in_bs = in_ld;
  if (!in_dev) {
    for (int b = 0; b < B; ++b) {
      char* dst = w->pinned_out + esz * (size_t)b * Nld;
      std::memcpy(dst, (const char*)d_in + esz * (size_t)b * (size_t)in_ld, esz * (size_t)samples[b]);
      std::memset(dst + esz * (size_t)samples[b], 0, esz * (Nld - (size_t)samples[b]));
    }
    HIPCHECK(hipMemcpyAsync(base + o_in, w->pinned_out, in_b, hipMemcpyHostToDevice, s));
    d_in = base + o_in;
    in_bs = (long long)Nld;
  }
  ResampleArgs a;
  std::memset(&a, 0, sizeof(a));
  a.in_f32 = in_f32 ? (const float*)d_in : nullptr;
  a.in_i16 = in_i16 ? (const short*)d_in : nullptr;
  a.in_bs = in_bs;
  a.samples = d_samples;
  a.table = rm->table;
  a.up = rm->p.up;
  a.down = rm->p.down;
  a.half_len = rm->p.half_len;
  a.Tp = rm->Tp;
  if (y_direct) {
    a.y = out_f32;
    a.y_bs = a.y_ld = out_ld;
  } else if (y_ws) {
    a.y = (float*)(base + o_y);
    a.y_bs = a.y_ld = (long long)Old;
  }
  short* const d_pcm = out_dev ? (short*)out_i16 : (short*)(base + o_pcm);  // where either launch leaves the int16 rows
  const long long pcm_ld = out_dev ? (long long)out_ld : (long long)Old;
  if (out_i16 && !normalize) {
    a.pcm = d_pcm;
    a.pcm_bs = a.pcm_ld = pcm_ld;
  }
  if (normalize) {
    a.peak = (float*)(base + o_peak);
    a.peak_ld = tiles;
  }
  {
    // the widest row the launch writes, zero tails included (never narrower than the longest row's outputs)
    const long long span = std::max(std::max(a.y ? a.y_ld : 0LL, a.pcm ? a.pcm_ld : 0LL), Omax);
    const dim3 grid((unsigned)((span + RS_TILE - 1) / RS_TILE), B);
    // the last lane's inputs end (up - 1 + 255 down) div up + Tp behind the tile's first staged one, at most
    const long long need = ((long long)a.up - 1 + (long long)(RS_TILE - 1) * a.down) / a.up + a.Tp;
    const bool staged = need <= RS_SPAN;
    a.stage_rounds = staged ? (int)((need + RS_TILE - 1) / RS_TILE) : 0;
    ProfScope ps(ctx, w, KC_SMALL, 2.0 * (double)total * rm->T);  // no counted kernel name: filed under "-" 
    if (in_i16 && staged) hipLaunchKernelGGL((resample_kernel<true, true>), grid, dim3(RS_TILE), 0, s, a);
    else if (in_i16) hipLaunchKernelGGL((resample_kernel<true, false>), grid, dim3(RS_TILE), 0, s, a);
    else if (staged) hipLaunchKernelGGL((resample_kernel<false, true>), grid, dim3(RS_TILE), 0, s, a);
    else hipLaunchKernelGGL((resample_kernel<false, false>), grid, dim3(RS_TILE), 0, s, a);
  }
  if (normalize) {
    const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((pcm_ld + 1023) / 1024, 1), 256);
    ProfScope ps(ctx, w, KC_SMALL, 0);
    hipLaunchKernelGGL(resample_pcm_kernel, dim3(gx, B), dim3(256), 0, s, a.y, a.y_bs, d_samples, a.up, a.down, a.peak, a.peak_ld, d_pcm,
                       pcm_ld, pcm_ld);
  }
  if (!out_dev) {
    // host outputs: device -> the worker's pinned staging (behind the input's) -> the caller's rows, zero-filled up to out_ld
    char* pf = w->pinned_out + in_b;
    char* pi = pf + f32_b;
    if (f32_b) HIPCHECK(hipMemcpyAsync(pf, a.y, f32_b, hipMemcpyDeviceToHost, s));
    if (i16_b) HIPCHECK(hipMemcpyAsync(pi, d_pcm, i16_b, hipMemcpyDeviceToHost, s));
    HIPCHECK(mi355_sync(s));
    HIPCHECK(hipGetLastError());
    return scatter_rows(rows, B, WavRows{(float*)pf, Old, (short*)pi, Old}, RowWriter{false, s});
  }
  HIPCHECK(mi355_sync(s));
  HIPCHECK(hipGetLastError());
  return 0;
}
