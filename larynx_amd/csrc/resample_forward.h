// mi355tts host runtime — resampling: the load, length and call entry points (kernels: resample.h)
// (one translation unit: included once by mi355tts.hip, after hifigan_forward.h for the row delivery it shares; the call frame,
// the model table and the waveform intake: host_call.h)
#pragma once

constexpr int RS_MAX_SAMPLES_LOG2 = 24;
constexpr long long RS_MAX_SAMPLES = 1LL << RS_MAX_SAMPLES_LOG2;
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
  return register_model(ctx, std::move(rm), model_out);
}

extern "C" int64_t mi355tts_resample_length(mi355tts_ctx* ctx, int model, int64_t samples) {
  if (!ctx) return fail(MI355TTS_ERR_INVALID, "null argument");
  std::shared_ptr<ResamplerModel> pin;
  CHECK(find_model(ctx, model, &pin));
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
  CHECK(find_model(ctx, model, &pin));
  const ResamplerModel* rm = pin.get();
  WaveIn in{in_f32, in_i16, samples, B, in_ld, (flags & MI355TTS_IN_DEVICE) != 0};
  CHECK(in.check("in_ld", RS_MAX_SAMPLES_LOG2));
  long long Omax = 0, total = 0;
  for (int b = 0; b < B; ++b) {
    const long long o = resample_len(rm, samples[b]);
    Omax = std::max(Omax, o);
    total += o;
  }
  if (out_ld < Omax) return fail(MI355TTS_ERR_INVALID, "out_ld %lld < %lld samples of the longest row", (long long)out_ld, Omax);
  if (samples_out)
    for (int b = 0; b < B; ++b) samples_out[b] = resample_len(rm, samples[b]);
  const bool out_dev = (flags & MI355TTS_OUT_DEVICE) != 0;
  const bool normalize = out_i16 && pcm_mode == MI355TTS_PCM_NORMALIZE;
  CallFrame f(ctx);
  CHECK(f.open());
  Worker* w = f.w;
  hipStream_t s = f.s;
  const OutRows rows = {nullptr, nullptr, 0, {out_f32, out_i16, out_ld, 0, 0, (size_t)Omax}};
  if (Omax == 0) return zero_outputs(f, rows, B, out_dev);
  CHECK(f.pinned_ints(B));
  // host rows travel through the workspace at strides in.Nld (in) and Old (out); device rows are read and written in place
  const size_t Old = (size_t)((Omax + 7) & ~7LL);
  const long long tiles = (Omax + RS_TILE - 1) / RS_TILE;
  const bool y_direct = out_dev && out_f32;              // the float rows straight into the caller's device buffer
  const bool y_ws = !y_direct && (out_f32 || normalize);  // or into the workspace: for the host copy, or for the second launch only
  Carver cv;
  in.carve(cv);
  const size_t o_y = cv.take(y_ws ? sizeof(float) * (size_t)B * Old : 0);
  const size_t o_pcm = cv.take(out_i16 && !out_dev ? sizeof(short) * (size_t)B * Old : 0);
  const size_t o_peak = cv.take(normalize ? sizeof(float) * (size_t)B * tiles : 0);
  // host outputs wait in the pinned staging behind the staged input
  const Staging st = host_staging(B, out_f32 && !out_dev, Old, out_i16 && !out_dev, Old, in.bytes);
  CHECK(f.reserve(cv.pos, st.end()));
  char* base = w->arena;
  CHECK(in.upload(f, w->pinned));
  int* const d_samples = in.d_samples;
  ResampleArgs a;
  std::memset(&a, 0, sizeof(a));
  a.in_f32 = in_f32 ? (const float*)in.d : nullptr;
  a.in_i16 = in_i16 ? (const short*)in.d : nullptr;
  a.in_bs = in.bs;
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
  return out_dev ? f.finish() : deliver_rows(f, rows, B, WavRows{a.y, Old, d_pcm, Old}, st, true);
}
