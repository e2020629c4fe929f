// mi355tts host runtime — resampling: the load, length and call entry points (kernels: resample.h)
// (one translation unit: included once by mi355tts.hip, after hifigan_forward.h; the model table, pack_polyphase and upload:
// host_call.h; the frame of the call, WaveCall, and the row delivery: host_rows.h)
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
  auto rm = std::make_shared<ResamplerModel>();
  rm->p = *params;
  rm->device = ctx->device;
  std::vector<float> table;
  CHECK(pack_polyphase(taps, params->half_len, up, RS_MAX_T, &rm->T, &rm->Tp, table));
  HIPCHECK(hipSetDevice(ctx->device));
  CHECK(upload(&rm->table, table, "resampler table"));
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
  WaveCall wc(ctx, in_f32, in_i16, samples, B, in_ld, out_f32, out_i16, out_ld, flags);
  CHECK(wc.check_args());
  if (!out_f32 && !out_i16) return fail(MI355TTS_ERR_INVALID, "no output: give out_f32, out_i16 or both");
  if (pcm_mode != MI355TTS_PCM_SATURATE && pcm_mode != MI355TTS_PCM_NORMALIZE) return fail(MI355TTS_ERR_INVALID, "unknown pcm_mode %d", pcm_mode);
  std::shared_ptr<ResamplerModel> pin;
  CHECK(find_model(ctx, model, &pin));
  const ResamplerModel* rm = pin.get();
  CHECK(wc.in.check("in_ld", RS_MAX_SAMPLES_LOG2));
  long long Omax = 0, total = 0;
  for (int b = 0; b < B; ++b) {
    const long long o = resample_len(rm, samples[b]);
    Omax = std::max(Omax, o);
    total += o;
  }
  CHECK(wc.check_out(Omax));
  if (samples_out)
    for (int b = 0; b < B; ++b) samples_out[b] = resample_len(rm, samples[b]);
  const bool normalize = out_i16 && pcm_mode == MI355TTS_PCM_NORMALIZE;
  CHECK(wc.open());
  Worker* w = wc.f.w;
  hipStream_t s = wc.f.s;
  if (Omax == 0) return wc.empty({});
  CHECK(wc.f.pinned_ints(B));
  // host rows travel through the workspace at strides in.Nld (in) and wc.Nld (out); device rows are read and written in place
  const long long tiles = (Omax + RS_TILE - 1) / RS_TILE;
  const bool y_ws = !out_f32 && normalize;  // float rows nobody receives: in the workspace, for the second launch only
  Carver cv = wc.carve();
  const size_t o_y = cv.take(y_ws ? sizeof(float) * (size_t)B * wc.Nld : 0);
  const size_t o_peak = cv.take(normalize ? sizeof(float) * (size_t)B * tiles : 0);
  CHECK(wc.reserve(cv));
  char* base = w->arena;
  ResampleArgs a;
  std::memset(&a, 0, sizeof(a));
  wc.in.bind(a);
  a.table = rm->table;
  a.up = rm->p.up;
  a.down = rm->p.down;
  a.half_len = rm->p.half_len;
  a.Tp = rm->Tp;
  if (out_f32) {
    a.y = wc.d_y;
    a.y_bs = a.y_ld = wc.ld;
  } else if (y_ws) {
    a.y = (float*)(base + o_y);
    a.y_bs = a.y_ld = (long long)wc.Nld;
  }
  if (out_i16 && !normalize) {  // (else the second launch leaves the int16 rows there)
    a.pcm = wc.d_pcm;
    a.pcm_bs = a.pcm_ld = wc.ld;
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
    const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((wc.ld + 1023) / 1024, 1), 256);
    ProfScope ps(ctx, w, KC_SMALL, 0);
    hipLaunchKernelGGL(resample_pcm_kernel, dim3(gx, B), dim3(256), 0, s, a.y, a.y_bs, a.samples, a.up, a.down, a.peak, a.peak_ld, wc.d_pcm,
                       wc.ld, wc.ld);
  }
  return wc.end();
}
