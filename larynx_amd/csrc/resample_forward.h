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

// ------------------------------------------------------------------ the launches, on an open wave call
// (shift_forward.h queues the same two behind its own kernels)
// What a stage's last float rows go through on their way out, the plan of mi355tts_resample: the f32 rows and / or the saturating
// int16 rows straight from the stage's kernel, or — normalised int16 — its float rows (in the workspace when nobody receives
// them) and the max |y| of every RS_TILE outputs, which resample_pcm_kernel turns into the int16 rows in a second launch.
struct WaveOutPlan {
  bool f32, i16, normalize, y_ws;
  long long tiles;
};
struct WaveOutTakes {
  size_t o_y, o_peak;
};
static WaveOutPlan wave_out_plan(const float* out_f32, const int16_t* out_i16, bool normalize, long long Omax) {
  return {out_f32 != nullptr, out_i16 != nullptr, normalize, !out_f32 && normalize, (Omax + RS_TILE - 1) / RS_TILE};
}
static WaveOutTakes wave_out_carve(Carver& cv, const WaveCall& wc, const WaveOutPlan& p) {
  WaveOutTakes t;
  t.o_y = cv.take(p.y_ws ? sizeof(float) * (size_t)wc.in.B * wc.Nld : 0);
  t.o_peak = cv.take(p.normalize ? sizeof(float) * (size_t)wc.in.B * p.tiles : 0);
  return t;
}
// y / pcm / peak of a stage's kernel arguments (ResampleArgs, ShiftOlaArgs), behind wc.reserve
template <class Args>
static void wave_out_bind(Args& a, const WaveCall& wc, const WaveOutPlan& p, const WaveOutTakes& t) {
  char* base = wc.f.w->arena;
  if (p.f32) {
    a.y = wc.d_y;
    a.y_bs = a.y_ld = wc.ld;
  } else if (p.y_ws) {  // float rows nobody receives: in the workspace, for the second launch only
    a.y = (float*)(base + t.o_y);
    a.y_bs = a.y_ld = (long long)wc.Nld;
  }
  if (p.i16 && !p.normalize) {  // (else the second launch leaves the int16 rows there)
    a.pcm = wc.d_pcm;
    a.pcm_bs = a.pcm_ld = wc.ld;
  }
  if (p.normalize) {
    a.peak = (float*)(base + t.o_peak);
    a.peak_ld = p.tiles;
  }
}
// resample_kernel on the rows `a` names (input and outputs bound by the caller): Omax outputs in the longest row, `total` in all
static void resample_launch(mi355tts_ctx* ctx, Worker* w, hipStream_t s, const ResamplerModel* rm, ResampleArgs& a, bool in_i16, long long Omax,
                            long long total, int B) {
  a.table = rm->table;
  a.up = rm->p.up;
  a.down = rm->p.down;
  a.half_len = rm->p.half_len;
  a.Tp = rm->Tp;
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
// resample_pcm_kernel: the float rows and tile peaks `a` names -> the call's normalised int16 rows
template <class Args>
static void resample_pcm_launch(mi355tts_ctx* ctx, Worker* w, hipStream_t s, const Args& a, const WaveCall& wc, int B, int up, int down,
                                const int* out_n) {
  const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((wc.ld + 1023) / 1024, 1), 256);
  ProfScope ps(ctx, w, KC_SMALL, 0);
  hipLaunchKernelGGL(resample_pcm_kernel, dim3(gx, B), dim3(256), 0, s, a.y, a.y_bs, a.samples, up, down, a.peak, a.peak_ld, wc.d_pcm, wc.ld,
                     wc.ld, out_n);
}
static void resample_pcm_launch(mi355tts_ctx* ctx, Worker* w, hipStream_t s, const ResampleArgs& a, const WaveCall& wc, int B) {
  resample_pcm_launch(ctx, w, s, a, wc, B, a.up, a.down, a.out_n);
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
  const WaveOutPlan plan = wave_out_plan(out_f32, out_i16, normalize, Omax);
  Carver cv = wc.carve();
  const WaveOutTakes tk = wave_out_carve(cv, wc, plan);
  CHECK(wc.reserve(cv));
  ResampleArgs a;
  std::memset(&a, 0, sizeof(a));
  wc.in.bind(a);
  wave_out_bind(a, wc, plan, tk);
  resample_launch(ctx, w, s, rm, a, in_i16 != nullptr, Omax, total, B);
  if (normalize) resample_pcm_launch(ctx, w, s, a, wc, B);
  return wc.end();
}
