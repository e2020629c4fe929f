// mi355tts host runtime — mi355tts_hifigan_infer: the HiFi-GAN layer schedule (hifi_gan/models.py:186-202) and the denoiser
// (one translation unit: included once by mi355tts.hip, after the kernel headers)
// The call struct and the workspace layout; VocPass (what a pass shares); the stage bookkeeping both precisions use (VocStage,
// StageCursor, chain_planes / step_dst, run_forked); the f32 / split-bf16 generator and the fp16 generator, each a walk over pre /
// upsample / resblocks / post; then hifigan_run: empty call, layout and bind, generate, denoise, deliver.  The row view of a call's
// outputs (OutRows) and the delivery (zero_outputs, deliver_rows) are host_rows.h's.
// Every call runs on a CallFrame (host_call.h): it holds the worker and drains the streams when a call fails midway.
#pragma once

// ------------------------------------------------------------------ HiFi-GAN forward
extern "C" int mi355tts_hifigan_hop(mi355tts_ctx* ctx, int vocoder) {
  if (!ctx) return fail(MI355TTS_ERR_INVALID, "ctx null");
  std::shared_ptr<HifiModel> vpin;
  CHECK(find_model(ctx, vocoder, &vpin));
  return vpin->hop;
}

// One vocoder call's outputs: per row [pad_before zeros][frames[b]*hop samples][zeros up to wav_ld]
// (the pads are the SSML pauses `_sentence_task` adds with np.pad, larynx/__init__.py:277-283).
struct VocCall {
  float denoiser_strength = 0.f;
  float* wav_f32 = nullptr;
  int16_t* wav_i16 = nullptr;
  int64_t wav_ld = 0;
  uint32_t flags = 0;
  int pad_before = 0, pad_after = 0;
  // optional, [B] (B <= VOC_MAX_ROWS): per-row destinations, strides and pauses; the five fields above are then unused
  const VocRow* rows = nullptr;
  // The model's precision for this call: read ONCE, by the call's first hifigan_precheck (mi355tts_model_set_precision may run on
  // another thread meanwhile); the bias pass, the generator and the denoiser's bias slot all follow this value.
  int precision = -1;
  VocTaps* taps = nullptr;  // mi355tts_hifigan_infer_taps: keep a copy of every plane the schedule writes (voc_tap); else null
};

static int ensure_denoiser_bias(mi355tts_ctx* ctx, HifiModel* hm, int vocoder, int precision);

// Checks that need no worker (and may run the one-time bias-spectrum pass on a worker of their own).  Fixes the call's precision.
static int hifigan_precheck(mi355tts_ctx* ctx, HifiModel* hm, int vocoder, const int32_t* frames, int B, int M, int Fmax, VocCall& c) {
  if (c.precision < 0) c.precision = hm->precision.load();
  if (M != hm->hp.num_mels) return fail(MI355TTS_ERR_INVALID, "mel has %d channels, vocoder expects %d", M, hm->hp.num_mels);
  if (c.rows) {  // per-row destinations: every row against its own frame count
    if (B > VOC_MAX_ROWS) return fail(MI355TTS_ERR_INVALID, "internal: %d rows with per-row outputs", B);
    for (int b = 0; b < B; ++b) {
      const VocRow& r = c.rows[b];
      if (r.pad_before < 0 || r.pad_after < 0) return fail(MI355TTS_ERR_INVALID, "negative pause padding");
      const long long need = (long long)(frames ? frames[b] : 0) * hm->hop + r.pad_before + r.pad_after;
      if (frames && r.wav_ld < need) return fail(MI355TTS_ERR_TOO_SMALL, "wav_ld %lld < %lld samples", (long long)r.wav_ld, need);
    }
  } else {
    if (c.pad_before < 0 || c.pad_after < 0) return fail(MI355TTS_ERR_INVALID, "negative pause padding");
    const long long need = (long long)Fmax * hm->hop + c.pad_before + c.pad_after;
    if (Fmax >= 0 && c.wav_ld < need) return fail(MI355TTS_ERR_TOO_SMALL, "wav_ld %lld < %lld samples", (long long)c.wav_ld, need);
  }
  if (c.denoiser_strength > 0.f && Fmax != 0) {
    // the reference's STFT needs more than one 1024-sample frame per utterance
    // (larynx/audio.py:232-249 raises on shorter input)
    if (frames)
      for (int b = 0; b < B; ++b)
        if ((long long)frames[b] * hm->hop <= DN_FFT)
          return fail(MI355TTS_ERR_INVALID, "utterance %d has %d frames: too short for the denoiser", b, frames[b]);
    CHECK(ensure_denoiser_bias(ctx, hm, vocoder, c.precision));
  }
  return 0;
}

// Workspace of one vocoder call (bytes, and where each piece sits).  ONE definition, used by the
// forward pass and by mi355tts_reserve.
struct HifiLayout {
  size_t plane = 0, Nld = 0, total = 0;
  int nbuf = 0, Tmax = 0;
  size_t o_buf[2 + 4 * 3], o_wav, o_i16, o_peak, o_wav2, o_fbuf;
};
static HifiLayout hifi_layout(const mi355tts_hifigan_hparams& h, int hop, int B, int F, bool denoise, bool split_out, int pads) {
  HifiLayout L;
  const int C0 = h.upsample_initial_channel;
  L.plane = (size_t)C0 * (size_t)((F + 3) & ~3);  // row strides are multiples of 4 floats (16-byte staging loads)
  long long len = F;
  for (int i = 0; i < h.num_upsamples; ++i) {
    len *= h.upsample_rates[i];
    L.plane = std::max(L.plane, (size_t)(C0 >> (i + 1)) * (size_t)((len + 3) & ~3LL));
  }
  const long long N = (long long)F * hop;
  L.Nld = (size_t)((N + 3) & ~3LL);
  L.nbuf = split_out ? 2 + 4 * h.num_kernels : 6;
  Carver cv;
  for (int i = 0; i < L.nbuf; ++i) L.o_buf[i] = cv.take(sizeof(float) * (size_t)B * L.plane);
  L.o_wav = cv.take(sizeof(float) * (size_t)B * L.Nld);
  L.o_i16 = cv.take(sizeof(short) * (size_t)B * (L.Nld + (size_t)pads));
  L.o_peak = cv.take(sizeof(float) * (size_t)B * (L.Nld / POST_TW + 2));  // post_conv_kernel's per-workgroup maxima of every row
  L.Tmax = denoise ? (int)((N - DN_FFT + DN_HOP - 1) / DN_HOP) : 0;
  L.o_wav2 = cv.take(denoise ? sizeof(float) * (size_t)B * L.Nld : 0);
  L.o_fbuf = cv.take(denoise ? sizeof(float) * (size_t)B * L.Tmax * DN_FFT : 0);
  L.total = cv.pos;
  return L;
}
static bool hifi_split_out(bool serial_branches, const mi355tts_hifigan_hparams& h) {
  return !serial_branches && h.num_kernels >= 2 && h.num_kernels <= 3;
}

// the rows of a vocoder call (host_rows.h)
static OutRows call_rows(const VocCall& c, const mi355tts_mel* mel, int hop) {
  if (c.rows) return {c.rows, mel->frames.data(), hop, {}};
  return {nullptr, nullptr, 0, {c.wav_f32, c.wav_i16, c.wav_ld, (size_t)c.pad_before, (size_t)c.pad_after, (size_t)mel->max_frames * hop}};
}

// ------------------------------------------------------------------ what one vocoder pass shares
// Both generators, the denoiser and the delivery take this one argument.  `bind` lays the workspace out and fills the pointers.
struct VocPass {
  CallFrame& frame;
  mi355tts_ctx* ctx;
  Worker* w;
  HifiModel* hm;
  const mi355tts_mel* mel;
  hipStream_t s;
  int B, F, hop;
  const int* d_frames;  // device, [B]
  int voc_host_len;     // the row's frame count at batch 1, else -1
  const CallOptions& opt;  // as read when the worker was checked out: a call never mixes schedules if an option changes while it runs
  int prec;                // as hifigan_precheck read it: the generator, the bias slot and the bias pass all see this value
  bool f16;                // the native fp16 generator: its own schedule, chains always write their own planes
  float denoiser_strength;
  bool denoise;
  // Option "voc_out" (default 1): conv_post + tanh + the rows' peaks in ONE dedicated launch and the delivery of the rows in one
  // more (voc_out.h); 0 = the generic conv tile, zero_tail, absmax, to_int16 and a copy / fill per piece of every row.
  bool voc_out = false;
  bool out_dev;  // MI355TTS_OUT_DEVICE
  int pads = 0;  // the longest pause pair of the call's rows, in samples
  bool any_f32 = false, any_i16 = false;
  // the workspace (hifi_layout)
  float* buf[2 + 4 * 3];  // plane buffers
  float *wav = nullptr, *wav2 = nullptr, *fbuf = nullptr;  // the f32 waveform rows [B][Nld]; the denoiser's output and frames
  short* i16 = nullptr;  // int16 staging rows [B][ild]
  size_t Nld = 0, ild = 0;
  int Tmax = 0;
  unsigned* peaks = nullptr;  // one |max| per row (absmax_kernel), or viewed as floats: `peak`
  // the dedicated conv_post kernels leave the per-workgroup maxima of the FINAL waveform (not behind the denoiser)
  float* peak = nullptr;  // [B][peak_ld], or null when nobody reads them
  long long peak_ld = 0;
  const float* bias_spec = nullptr;
  Staging staged;  // host outputs: rows of the samples alone / of samples + pauses (nothing for MI355TTS_OUT_DEVICE)
  VocTaps* taps;   // the test seam (voc_tap): null in every call but mi355tts_hifigan_infer_taps'

  VocPass(CallFrame& f, HifiModel* hm_, const mi355tts_mel* mel_, const VocCall& call)
      : frame(f), ctx(f.ctx), w(f.w), hm(hm_), mel(mel_), s(f.s), B(mel_->B), F(mel_->max_frames), hop(hm_->hop), d_frames(mel_->frames_dev),
        voc_host_len(mel_->B == 1 ? mel_->frames[0] : -1), opt(f.w->opt), prec(call.precision), f16(call.precision == MI355TTS_PRECISION_F16),
        denoiser_strength(call.denoiser_strength), denoise(call.denoiser_strength > 0.f && mel_->max_frames > 0),
        out_dev((call.flags & MI355TTS_OUT_DEVICE) != 0), taps(call.taps) {}

  RowLen rows(int mul) const { return row_len(B, voc_host_len, d_frames, mul); }
  template <class P>
  P* plane(int i) const { return reinterpret_cast<P*>(buf[i]); }

  int bind(const VocCall& call, const OutRows& out) {
    const mi355tts_hifigan_hparams& h = hm->hp;
    if (f16 && !hm->f16_ok) return fail(MI355TTS_ERR_INVALID, "internal: fp16 mode on a vocoder it does not cover");
    bias_spec = hm->bias_spec[f16 ? 1 : 0];
    if (denoise && !bias_spec) return fail(MI355TTS_ERR_INVALID, "internal: no denoiser bias for this precision");
    voc_out = f16 || (!opt.env.voc_out_off && opt.voc_out && hm->post_C == (h.upsample_initial_channel >> h.num_upsamples) && hm->post.K == 7);
    if (call.rows && !voc_out) return fail(MI355TTS_ERR_INVALID, "internal: per-row outputs need the voc_out tail");
    for (int b = 0; b < B; ++b) {
      const OutRow r = out(b);
      pads = std::max(pads, (int)(r.pad_before + r.pad_after));
      any_f32 = any_f32 || r.f32;
      any_i16 = any_i16 || r.i16;
    }
    const HifiLayout lay = hifi_layout(h, hop, B, F, denoise, f16 || hifi_split_out(opt.serial_branches, h), pads);
    if (f16 && (size_t)((mel->M + 7) / 8) * F * 16 > lay.plane * sizeof(float)) return fail(MI355TTS_ERR_INVALID, "internal: mel octets exceed a plane buffer");
    // a pageable destination would make every hipMemcpyAsync a blocking staged copy: host rows travel through pinned staging
    staged = host_staging(B, any_f32 && !out_dev, (size_t)F * hop, any_i16 && !out_dev, (size_t)F * hop + (size_t)pads);
    CHECK(frame.reserve(lay.total, staged.end()));
    char* base = w->arena;
    for (int i = 0; i < lay.nbuf; ++i) buf[i] = (float*)(base + lay.o_buf[i]);
    wav = (float*)(base + lay.o_wav);
    wav2 = (float*)(base + lay.o_wav2);
    fbuf = (float*)(base + lay.o_fbuf);
    i16 = (short*)(base + lay.o_i16);
    peaks = (unsigned*)(base + lay.o_peak);
    Nld = lay.Nld;
    ild = Nld + (size_t)pads;
    Tmax = lay.Tmax;
    peak_ld = (long long)(Nld / POST_TW + 2);
    peak = voc_out && any_i16 && !denoise ? reinterpret_cast<float*>(peaks) : nullptr;
    return 0;
  }
};

// ------------------------------------------------------------------ the test seam: the planes of one call
// A copy of the plane the last launch on `p.s` wrote — `ch` channels at row stride `ld`, rows of frames x `mul` columns, fp16 octet
// planes or f32 rows — queued on the same stream right behind that launch (host_taps.h).  Callers test `p.taps` first.
static int voc_tap(VocPass& p, const std::string& name, const void* x, bool f16, int ch, int ld, int mul) {
  std::vector<int> len;
  for (int b = 0; b < p.B; ++b) len.push_back((int)std::min<long long>((long long)p.mel->frames[b] * mul, ld));
  // a plane with no counted launch since the tap before it (a `.t` plane, the second of two sums) is filed under that tap's launch
  return p.taps->add(p.s, name, x, f16, p.B, ch, ld, len.data(), p.taps->last_kn < 0);
}

// ------------------------------------------------------------------ stage bookkeeping, shared by both precisions
// Stage i as its upsampler writes it and its ResBlocks keep it: `cout` channels, `Lout` columns at row stride `ldo`, `bs` plane
// units per batch row, lengths = frames x `mul`.  The f32 / split-bf16 planes are floats with row strides rounded to 4 (16-byte
// staging loads); the fp16 planes are 16-byte octets of 8 channels, un-rounded.
struct VocStage {
  int i, u, ku, cout, Lout, ldo, mul;
  long long bs;
};
static VocStage voc_stage(const mi355tts_hifigan_hparams& h, int i, int Lin, int mul, bool f16) {
  VocStage st;
  st.i = i;
  st.u = h.upsample_rates[i];
  st.ku = h.upsample_kernel_sizes[i];
  st.cout = h.upsample_initial_channel >> (i + 1);
  st.Lout = Lin * st.u;
  st.ldo = f16 ? st.Lout : (st.Lout + 3) & ~3;
  st.mul = mul * st.u;
  st.bs = f16 ? (long long)(st.cout / 8) * st.ldo : (long long)st.cout * st.ldo;
  return st;
}

// The input of the next stage (or of conv_post): (cur[0] + ... + cur[ncur-1]) / div — `cur[0]` alone, or the chain outputs still to
// be averaged by the consumer's staging load — of `ch` channels, `Lin` columns at row stride `ldin`, lengths = frames x `mul`.
template <class P>  // float, or uint4 for the fp16 octet planes
struct StageCursor {
  P* cur[3] = {nullptr, nullptr, nullptr};
  int ncur = 1;
  float div = 1.0f;
  int ch = 0, Lin = 0, ldin = 0, mul = 1;
  int flip = 0;  // which half of the chain-output buffers the next stage writes

  // x / x2 / x3 / in_div of a consumer (ConvArgs, PostArgs, HConvArgs, HPostArgs); with one plane, in_div stays the caller's
  template <class Args>
  void inputs(Args& a) const {
    a.x = cur[0];
    if (ncur > 1) {
      a.x2 = cur[1];
      a.x3 = ncur > 2 ? cur[2] : nullptr;
      a.in_div = div;
    }
  }
  // after stage `st`: its `n` outputs, to be summed and divided by `d`.  The three continuations: the chains' own outputs (n = nk,
  // d = nk, flipped), the serial form's one averaged plane (n = 1, d = 1), mrf_small's two sums (n = 2, d = nk).
  void advance(const VocStage& st, P* const* outs, int n, float d, bool flipped) {
    for (int j = 0; j < 3; ++j) cur[j] = j < n ? outs[j] : nullptr;
    ncur = n;
    div = d;
    ch = st.cout;
    Lin = st.Lout;
    ldin = st.ldo;
    mul = st.mul;
    if (flipped) flip ^= 1;
  }
};

// The planes of ResBlock chain j in a stage: conv1's output, the ping / pong planes of the dilation steps, the chain's output.
template <class P>
struct ChainPlanes {
  P *t, *ping, *pong, *dst_last;
};
template <class P>
static ChainPlanes<P> chain_planes(const VocPass& p, int j, int flip, bool split_out) {
  // serial form: the chains share their scratch planes and accumulate into one output
  if (!split_out) return {p.plane<P>(2), p.plane<P>(3), p.plane<P>(4), p.plane<P>(5)};
  // per-chain scratch: buf[2 + 4j .. 2 + 4j + 3] = {t, ping, out(flip 0), out(flip 1)}.  pong is the last stage's output: dead
  // once the upsampler (before the fork) has read it
  const int k = 2 + 4 * j;
  return {p.plane<P>(k), p.plane<P>(k + 1), p.plane<P>(k + 2 + (flip ^ 1)), p.plane<P>(k + 2 + flip)};
}
// where dilation step d of nd writes
template <class P>
static P* step_dst(const ChainPlanes<P>& c, int d, int nd) {
  return d == nd - 1 ? c.dst_last : (d & 1) ? c.pong : c.ping;
}

// `body` with `n_side` of the worker's side streams forked off `s` before it and joined behind it (0: `body` alone).  One
// function, so that no later edit separates a record from its wait; an error return leaves the streams to the call frame.
template <class Body>
static int run_forked(Worker* w, hipStream_t s, int n_side, Body&& body) {
  if (n_side > 0) {
    HIPCHECK(hipEventRecord(w->ev_fork, s));
    for (int j = 0; j < n_side; ++j) HIPCHECK(hipStreamWaitEvent(w->aux[j], w->ev_fork, 0));
  }
  CHECK(body());
  for (int j = 0; j < n_side; ++j) {
    HIPCHECK(hipEventRecord(w->ev_join[j], w->aux[j]));
    HIPCHECK(hipStreamWaitEvent(s, w->ev_join[j], 0));
  }
  return 0;
}

// ------------------------------------------------------------------ the f32 / split-bf16 generator, conv_pre .. conv_post + tanh
// How the ResBlock chains of every stage of this pass go out
struct F32Schedule {
  bool split_out, grouped, concurrent;
  int rb_tiles;
};
static int f32_schedule(const VocPass& p, F32Schedule& sc) {
  const mi355tts_hifigan_hparams& h = p.hm->hp;
  const CallOptions& opt = p.opt;
  Worker* w = p.w;
  // The nk ResBlock chains of a stage are independent (MRF).  Each chain writes its own
  // output and the average is taken by the consumer's staging load (`split_out`).  A call
  // that has the GPU to itself also runs the chains on separate streams so their workgroups
  // interleave — at batch 1 one conv launch has fewer tiles than the chip has SIMDs
  // (`concurrent`); when other calls are in flight they fill the chip, and forking would only
  // make 3 x calls streams contend for the runtime's 4 hardware queues, so the call stays on
  // one stream (measured: 3-6 calls in flight, +8 % utterances/s).  Both forms compute the
  // same values in the same order: results do not depend on the load.
  // `serial_branches` (profiling / tests) additionally folds the average into the chains'
  // last epilogues (in-place accumulation, one output buffer).
  sc.split_out = hifi_split_out(opt.serial_branches, h);
  // grouped (default): the chains stay on ONE stream and the same-geometry launches of a step go out as
  // one grouped launch (conv_group_kernel / pair_group_kernel) — the chip is filled from one launch, with
  // no stream fork/join and independently of what else is in flight.  "mrf_group" = 0 restores the
  // round-1 schedule (fork onto three streams while the call has the GPU to itself).
  // "adaptive_schedule" = 1 sends the members out one by one while other calls are in flight.  That was worth
  // +3 % utterances/s at 6 calls in flight with the round-2 mid-way kernels; with the final tiles the grouped
  // launch wins under load too (f32 +1.3 %, split-bf16 +5 %, same box), so the option is off by default.
  // Every form runs the same tiles with the same code: results do not depend on the load.
  const bool busy = opt.adaptive_schedule && p.ctx->active_calls.load(std::memory_order_relaxed) > 1;
  sc.grouped = sc.split_out && h.num_kernels == 3 && opt.mrf_group && !busy;
  sc.concurrent = sc.split_out && !opt.mrf_group && !busy;
  if (p.taps && sc.concurrent)
    return fail(MI355TTS_ERR_INVALID, "taps: the forked schedule (\"mrf_group\" = 0) runs its chains on side streams a copy cannot be ordered behind");
  if (sc.concurrent && !w->aux[0]) {
    for (int i = 0; i < 2; ++i) {
      HIPCHECK(hipStreamCreateWithFlags(&w->aux[i], hipStreamNonBlocking));
      HIPCHECK(hipEventCreateWithFlags(&w->ev_join[i], hipEventDisableTiming));
    }
    HIPCHECK(hipEventCreateWithFlags(&w->ev_fork, hipEventDisableTiming));
  }
  // One workgroup target for the ResBlock launches in every schedule: the tile shape fixes the
  // k-split and with it the summation order, so a load-dependent choice would make results
  // depend on the load.  (With the final tile set 300, 700 and 1024 measured the same within
  // noise for the forked schedule.)  Tuning knob: MI355TTS_RB_TILES.
  sc.rb_tiles = opt.env.rb_tiles > 0 ? opt.env.rb_tiles : 1024;
  return 0;
}

static int f32_pre(VocPass& p, StageCursor<float>& c) {  // conv_pre (models.py:187)
  const int C0 = p.hm->hp.upsample_initial_channel, Fp = (p.F + 3) & ~3;
  c.cur[0] = p.buf[0];
  c.ch = C0;
  c.Lin = p.F;
  c.ldin = Fp;
  ConvArgs a = base_args(p.mel->voc, (long long)p.mel->M * p.mel->ld, p.mel->ld, p.d_frames, 1, c.cur[0], (long long)C0 * Fp, Fp, p.d_frames, 1, 1, 3);
  if (p.taps) CHECK(voc_tap(p, "mel", p.mel->voc, false, p.mel->M, p.mel->ld, 1));
  CHECK(launch_conv(p.ctx, p.w, p.hm->pre, a, EPI_LINEAR, p.B, p.F, KC_VOC_IO, nullptr, 1024, p.voc_host_len));
  if (p.taps) CHECK(voc_tap(p, "pre", c.cur[0], false, C0, Fp, 1));
  return 0;
}

static int f32_upsample(VocPass& p, const StageCursor<float>& c, const VocStage& st) {  // x = ups[i](leaky_relu(x, 0.1))  (models.py:189-190)
  ConvArgs a = base_args(c.cur[0], (long long)c.ch * c.ldin, c.ldin, p.d_frames, c.mul, p.buf[1], st.bs, st.ldo, p.d_frames, st.mul, 1, st.ku / st.u - 1);
  c.inputs(a);
  a.in_slope = 0.1f;
  a.up = st.u;
  a.up_pad = (st.ku - st.u) / 2;
  CHECK(launch_conv(p.ctx, p.w, p.hm->ups[st.i], a, EPI_UPSAMPLE, p.B, c.Lin + st.ku / st.u - 1, KC_UPSAMPLE, nullptr, 1024, p.voc_host_len, p.prec));
  if (p.taps) CHECK(voc_tap(p, tap_name("up%d", st.i), p.buf[1], false, st.cout, st.ldo, st.mul));
  return 0;
}

// One dilation step of one MRF chain, planned: the fused pair if its geometry is covered, else conv1 (+ conv2)
struct VocStep {
  PairPlan pair;
  ConvPlan c1, c2;
  float* dst;
};
// The same step of the three chains as grouped launches on stream `s`: all fused pairs give one pair group, no pairs give one conv
// group for conv1 and one for conv2.  Returns 0 = launched, 1 = not groupable (the caller runs the members one by one), < 0 = error.
static int run_step_grouped(mi355tts_ctx* ctx, Worker* w, const VocStep (&sp)[3], hipStream_t s) {
  const int npair = sp[0].pair.ok + sp[1].pair.ok + sp[2].pair.ok;
  if (npair == 3) {
    const PairPlan* pairs[3] = {&sp[0].pair, &sp[1].pair, &sp[2].pair};
    return run_pair_group(ctx, w, pairs, 3, s);
  }
  if (npair != 0) return 1;
  const ConvPlan* c1[3] = {&sp[0].c1, &sp[1].c1, &sp[2].c1};
  const ConvPlan* c2[3] = {&sp[0].c2, &sp[1].c2, &sp[2].c2};
  const int rc = run_group(ctx, w, c1, 3, s);
  if (rc != 0 || sp[0].c2.empty) return rc;
  const int rc2 = run_group(ctx, w, c2, 3, s);
  if (rc2 == 1)
    for (int j = 0; j < 3; ++j) CHECK(run_plan(ctx, w, sp[j].c2, s));
  return rc2 < 0 ? rc2 : 0;
}

// The nk chains of one stage (MRF: resblocks on the same input, models.py:191-197): their planes, running inputs and streams
struct F32Chains {
  VocPass& p;
  const F32Schedule& sc;
  const VocStage& st;
  int nk, nd;
  ChainPlanes<float> pl[MI355TTS_MAX_STAGES];
  const float* rin[MI355TTS_MAX_STAGES];
  hipStream_t stream[MI355TTS_MAX_STAGES];

  F32Chains(VocPass& p_, const F32Schedule& sc_, const VocStage& st_, int flip)
      : p(p_), sc(sc_), st(st_), nk(p_.hm->hp.num_kernels), nd(p_.hm->hp.num_dilations) {
    for (int j = 0; j < nk; ++j) {
      pl[j] = chain_planes<float>(p, j, flip, sc.split_out);
      rin[j] = p.buf[1];
      stream[j] = (sc.concurrent && j > 0) ? p.w->aux[j - 1] : p.s;
    }
  }

  int plan_step(int j, int d, VocStep& sp) const {
    const mi355tts_hifigan_hparams& h = p.hm->hp;
    const HifiResConv& rc = p.hm->rb[st.i][j][d];
    const int kk = h.resblock_kernel_sizes[j], B = p.B, ldo = st.ldo, mul = st.mul, Lout = st.Lout, host_len = p.voc_host_len;
    const long long bs = st.bs;
    const int* d_frames = p.d_frames;
    const float* x = rin[j];
    const float inv_nk = 1.0f / (float)nk;
    sp.dst = step_dst(pl[j], d, nd);
    if (!sp.dst) return fail(MI355TTS_ERR_INVALID, "internal: resblock scratch aliasing");
    const bool fold = d == nd - 1 && !sc.split_out;  // serial form: the MRF average is folded into the chains' last epilogues
    sp.pair.ok = false;
    if (h.resblock_type == 1) {  // ResBlock1.forward, models.py:91-98
      plan_pair(p.opt, rc.c1, rc.c2, x, sp.dst, bs, ldo, d_frames, mul, rc.dil, fold ? inv_nk : 1.0f, fold ? (j > 0) : 0, B, Lout, host_len,
                &sp.pair, p.prec);
      if (sp.pair.ok) return 0;
      ConvArgs a = base_args(x, bs, ldo, d_frames, mul, pl[j].t, bs, ldo, d_frames, mul, rc.dil, (kk * rc.dil - rc.dil) / 2);
      a.in_slope = 0.1f;
      CHECK(plan_conv(p.opt, rc.c1, a, EPI_LINEAR, B, Lout, KC_RESBLOCK, sc.rb_tiles, host_len, &sp.c1, p.prec));
      ConvArgs c2 = base_args(pl[j].t, bs, ldo, d_frames, mul, sp.dst, bs, ldo, d_frames, mul, 1, (kk - 1) / 2);
      c2.in_slope = 0.1f;
      c2.res = x;
      if (fold) {
        c2.alpha = inv_nk;
        c2.accum = j > 0;
      }
      CHECK(plan_conv(p.opt, rc.c2, c2, EPI_LINEAR, B, Lout, KC_RESBLOCK, sc.rb_tiles, host_len, &sp.c2, p.prec));
    } else {  // ResBlock2.forward, models.py:136-141
      ConvArgs a = base_args(x, bs, ldo, d_frames, mul, sp.dst, bs, ldo, d_frames, mul, rc.dil, (kk * rc.dil - rc.dil) / 2);
      a.in_slope = 0.1f;
      a.res = x;
      if (fold) {
        a.alpha = inv_nk;
        a.accum = j > 0;
      }
      CHECK(plan_conv(p.opt, rc.c1, a, EPI_LINEAR, B, Lout, KC_RESBLOCK, sc.rb_tiles, host_len, &sp.c1, p.prec));
      sp.c2.empty = true;
    }
    return 0;
  }
  // the planes step d of chain j left: conv1's output where the step materialised it, and the step's own output (the serial
  // form's last steps accumulate into the stage's average instead: tapped as "stage{i}" once the last chain has added its share)
  int tap_step(int j, int d, const VocStep& sp) const {
    const bool fold = d == nd - 1 && !sc.split_out;
    if (!sp.pair.ok && !sp.c2.empty) CHECK(voc_tap(p, tap_name("rb%d.%d.%d.t", st.i, j, d), pl[j].t, false, st.cout, st.ldo, st.mul));
    if (!fold) return voc_tap(p, tap_name("rb%d.%d.%d", st.i, j, d), sp.dst, false, st.cout, st.ldo, st.mul);
    return j == nk - 1 ? voc_tap(p, tap_name("stage%d", st.i), sp.dst, false, st.cout, st.ldo, st.mul) : 0;
  }
  int run_step_alone(int j, const VocStep& sp) const {
    if (sp.pair.ok) return run_pair(p.ctx, p.w, sp.pair, stream[j]);
    CHECK(run_plan(p.ctx, p.w, sp.c1, stream[j]));
    return run_plan(p.ctx, p.w, sp.c2, stream[j]);
  }
  // dilation-major: step d of every chain before step d + 1 of any — the chains have their own
  // buffers, and the same-geometry launches of a step can go out as ONE grouped launch
  int run_dilation_major() {
    for (int d = 0; d < nd; ++d) {
      VocStep sp[3];
      for (int j = 0; j < nk; ++j) CHECK(plan_step(j, d, sp[j]));
      if (nk == 3 && !sp[0].pair.ok && !sp[1].pair.ok && !sp[2].pair.ok) {  // tile shape of the step: before the schedule is chosen
        ConvPlan* c1s[3] = {&sp[0].c1, &sp[1].c1, &sp[2].c1};
        ConvPlan* c2s[3] = {&sp[0].c2, &sp[1].c2, &sp[2].c2};
        promote_group_plans(p.opt, c1s, nk);
        promote_group_plans(p.opt, c2s, nk);
      }
      const int rc = sc.grouped ? run_step_grouped(p.ctx, p.w, sp, p.s) : 1;
      if (rc < 0) return rc;
      if (rc == 1)
        for (int j = 0; j < nk; ++j) CHECK(run_step_alone(j, sp[j]));
      if (p.taps)
        for (int j = 0; j < nk; ++j) CHECK(tap_step(j, d, sp[j]));
      for (int j = 0; j < nk; ++j) rin[j] = sp[j].dst;
    }
    return 0;
  }
  // chain-major (the chains share their scratch planes and accumulate into one output)
  int run_chain_major() {
    for (int j = 0; j < nk; ++j)
      for (int d = 0; d < nd; ++d) {
        VocStep sp;
        CHECK(plan_step(j, d, sp));
        CHECK(run_step_alone(j, sp));
        if (p.taps) CHECK(tap_step(j, d, sp));
        rin[j] = sp.dst;
      }
    return 0;
  }
};

static int f32_resblocks(VocPass& p, const F32Schedule& sc, StageCursor<float>& c, const VocStage& st) {
  HifiModel* hm = p.hm;
  const int nk = hm->hp.num_kernels;
  if (p.opt.mrf_small && !p.opt.serial_branches && st.i < (int)hm->mrf.size() && hm->mrf[st.i].ok) {
    // narrow stage (C = 8 / 16): the three chains in ONE launch on LDS-resident tiles, written as two sums
    // (k = 3 + k = 7, and k = 11) that the consumer adds and divides by nk on load.  The stage-input plane and
    // the previous stage's chain outputs are dead once the upsampler has read them.
    float* sums[2] = {p.buf[0], p.buf[2]};
    CHECK(run_mrf_small(p.ctx, p.w, hm->mrf[st.i], hm->arena, p.buf[1], sums[0], sums[1], st.bs, st.ldo, p.d_frames, st.mul, p.B, st.Lout, p.voc_host_len, p.s));
    if (p.taps)  // the launch keeps its chains in LDS: only the two sums reach memory
      for (int m = 0; m < 2; ++m) CHECK(voc_tap(p, tap_name("stage%d.sum%d", st.i, m), sums[m], false, st.cout, st.ldo, st.mul));
    c.advance(st, sums, 2, (float)nk, false);
    return 0;
  }
  F32Chains chains(p, sc, st, c.flip);
  CHECK(run_forked(p.w, p.s, sc.concurrent ? nk - 1 : 0, [&] { return sc.split_out ? chains.run_dilation_major() : chains.run_chain_major(); }));
  if (sc.split_out) {
    float* outs[3] = {nullptr, nullptr, nullptr};
    for (int j = 0; j < nk; ++j) outs[j] = chains.pl[j].dst_last;
    c.advance(st, outs, nk, (float)nk, true);
  } else {
    // serial: buf[5] holds the averaged sum; rotate it with the stage-input buffer
    std::swap(p.buf[5], p.buf[0]);
    c.advance(st, &p.buf[0], 1, 1.0f, false);
  }
  return 0;
}

// what post_conv_kernel's and post_f16_kernel's arguments share; `x_bs` in the plane's units
template <class Args, class P>
static Args post_args(const VocPass& p, const StageCursor<P>& c, long long x_bs) {
  Args a;
  std::memset(&a, 0, sizeof(a));
  a.in_div = 1.0f;
  c.inputs(a);
  a.slope = 0.01f;
  a.x_bs = x_bs;
  a.x_ld = c.ldin;
  p.rows(c.mul).into(a);
  a.len_mul = c.mul;
  a.w = p.hm->arena + p.hm->post_w_off;
  a.bias = p.hm->arena + p.hm->post_b_off;
  a.C = c.ch;
  a.y = p.wav;
  a.y_bs = (long long)p.Nld;
  return a;
}

static int f32_post(VocPass& p, const StageCursor<float>& c) {  // x = tanh(conv_post(leaky_relu(x)))  — default slope 0.01 (models.py:198-200)
  if (!p.voc_out) {
    ConvArgs a = base_args(c.cur[0], (long long)c.ch * c.ldin, c.ldin, p.d_frames, c.mul, p.wav, (long long)p.Nld, (int)p.Nld, p.d_frames, c.mul, 1, 3);
    c.inputs(a);
    a.in_slope = 0.01f;
    a.out_act = ACT_TANH;
    CHECK(launch_conv(p.ctx, p.w, p.hm->post, a, EPI_LINEAR, p.B, c.Lin, KC_VOC_IO, nullptr, 1024, p.voc_host_len));
    if (p.taps) CHECK(voc_tap(p, "wav", p.wav, false, 1, (int)p.Nld, c.mul));
    return 0;
  }
  PostArgs a = post_args<PostArgs>(p, c, (long long)c.ch * c.ldin);
  if (p.peak) {
    a.peak = p.peak;
    a.peak_ld = p.peak_ld;
  }
  {
    ProfScope ps(p.ctx, p.w, KC_VOC_IO, 2.0 * (double)c.ch * 7 * (double)c.Lin * p.B);
    ps.kernel(KN_POST_CONV);
    const dim3 pg((c.Lin + POST_TW - 1) / POST_TW, p.B);
    switch_const<1, 2, 3>(c.ncur, [&](auto n) { hipLaunchKernelGGL(HIP_KERNEL_NAME(post_conv_kernel<7, decltype(n)::value>), pg, dim3(256), 0, p.s, a); });
  }
  if (p.taps) CHECK(voc_tap(p, "wav", p.wav, false, 1, (int)p.Nld, c.mul));
  return 0;
}

// Leaves the f32 waveform rows in `p.wav` ([B][Nld]) and, when asked (`voc_out` tail only), the |max| of every POST_TW-sample
// tile in `p.peak` — what hifigan_body_f16 leaves.
static int hifigan_body_f32(VocPass& p) {
  F32Schedule sc;
  CHECK(f32_schedule(p, sc));
  StageCursor<float> c;
  CHECK(f32_pre(p, c));
  for (int i = 0; i < p.hm->hp.num_upsamples; ++i) {
    const VocStage st = voc_stage(p.hm->hp, i, c.Lin, c.mul, false);
    CHECK(f32_upsample(p, c, st));
    CHECK(f32_resblocks(p, sc, c, st));
  }
  return f32_post(p, c);
}

// ------------------------------------------------------------------ the fp16 generator (packing, plans and launches: hifigan_f16.h)
// The same walk with its own rules: an fp16 plane of the same channels takes half of a plane buffer and its row stride is not
// rounded; conv1 stores its activated output; the chains always write their own planes on ONE stream (no serial or forked form).
// an fp16 plane: [B][ch / 8][ld] octets of 8 channels, row lengths = frames x mul
struct HPlane {
  uint4* x;
  int ch, ld, mul;
};
// a conv in -> out: no residual, no activation on either side, one input plane until the caller says otherwise
static HConvArgs f16_conv_args(const VocPass& p, const HPlane& in, const HPlane& out, int dil, int pad) {
  HConvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.x = in.x;
  a.x_bs = (long long)(in.ch / 8) * in.ld;
  a.x_ld = in.ld;
  a.in_div = 1.0f;
  a.dil = dil;
  a.pad = pad;
  a.in_slope = 1.0f;
  a.out_slope = 1.0f;
  a.y = out.x;
  a.y_bs = (long long)(out.ch / 8) * out.ld;
  a.y_ld = out.ld;
  a.cout = out.ch;
  h_set_lengths(a, p.B, p.d_frames, p.voc_host_len, in.mul, out.mul);
  return a;
}

static int f16_pre(VocPass& p, StageCursor<uint4>& c) {
  const mi355tts_mel* mel = p.mel;
  const int B = p.B, F = p.F, M = mel->M, moct = (M + 7) / 8, C0 = p.hm->hp.upsample_initial_channel;
  // mel [B][M][ld] f32 -> octet planes (buf[1]: free until the first upsampler writes it)
  uint4* melh = p.plane<uint4>(1);
  {
    ProfScope ps(p.ctx, p.w, KC_SMALL, 0, p.s);
    ps.kernel(KN_PACK_OCTETS);
    hipLaunchKernelGGL(pack_octets_kernel, dim3((F + 255) / 256, moct, B), dim3(256), 0, p.s, mel->voc, (long long)mel->M * mel->ld, mel->ld, M, p.d_frames, 1,
                       melh, (long long)moct * F, F);
  }
  if (p.taps) CHECK(voc_tap(p, "mel", melh, true, 8 * moct, F, 1));
  c.cur[0] = p.plane<uint4>(0);
  c.ch = C0;
  c.Lin = c.ldin = F;
  const HConvArgs a = f16_conv_args(p, {melh, 8 * moct, F, 1}, {c.cur[0], C0, F, 1}, 1, 3);  // conv_pre (models.py:187)
  const HPlan pl = plan_f16(p.hm->h_pre, a, EPI_LINEAR, B, F, 2.0 * C0 * M * 7 * (double)F * B);
  CHECK(run_plan_f16(p.ctx, p.w, pl, KC_VOC_IO, p.s));
  if (p.taps) CHECK(voc_tap(p, "pre", c.cur[0], true, C0, F, 1));
  return 0;
}

// x = ups[i](leaky_relu(x, 0.1))  (models.py:189-190); the MRF average of the previous stage is taken on load
static int f16_upsample(VocPass& p, const StageCursor<uint4>& c, const VocStage& st) {
  HConvArgs a = f16_conv_args(p, {c.cur[0], c.ch, c.ldin, c.mul}, {p.plane<uint4>(1), st.cout, st.ldo, st.mul}, 1, 1);
  c.inputs(a);
  a.in_slope = 0.1f;
  a.up = st.u;
  a.up_pad = st.u / 2;
  HPlan pl = plan_f16(p.hm->h_ups[st.i], a, EPI_UPSAMPLE, p.B, c.Lin + 1, 2.0 * c.ch * st.cout * (2.0 * st.u) * (double)c.Lin * p.B);
  pl.mrf = c.ncur > 1;
  CHECK(run_plan_f16(p.ctx, p.w, pl, KC_UPSAMPLE, p.s));
  if (p.taps) CHECK(voc_tap(p, tap_name("up%d", st.i), p.plane<uint4>(1), true, st.cout, st.ldo, st.mul));
  return 0;
}

// the fused form of a ResBlock1 step (pair_f16.h)
static HPairArgs f16_pair_args(const VocPass& p, const VocStage& st, const HResConv& rc, uint4* x, uint4* y, int dil) {
  HPairArgs a;
  std::memset(&a, 0, sizeof(a));
  a.x = x;
  a.y = y;
  a.bs = st.bs;
  a.ld = st.ldo;
  p.rows(st.mul).into(a);
  a.len_mul = st.mul;
  a.w1 = rc.c1.w;
  a.b1 = rc.c1.bias;
  a.nslab1 = rc.c1.nslab;
  a.w2 = rc.c2.w;
  a.b2 = rc.c2.bias;
  a.nslab2 = rc.c2.nslab;
  a.C = st.cout;
  a.dil = dil;
  a.slope = 0.1f;
  return a;
}

static int f16_resblocks(VocPass& p, StageCursor<uint4>& c, const VocStage& st) {
  const mi355tts_hifigan_hparams& h = p.hm->hp;
  const int nk = h.num_kernels, nd = h.num_dilations, B = p.B, ch = st.cout, Lout = st.Lout;
  ChainPlanes<uint4> pl[3];
  uint4* rin[3];
  auto plane = [&](uint4* x) { return HPlane{x, ch, st.ldo, st.mul}; };
  for (int j = 0; j < nk; ++j) {
    pl[j] = chain_planes<uint4>(p, j, c.flip, true);
    rin[j] = p.plane<uint4>(1);
  }
  // in this mode "mrf_group" and "rb_pair" select the grouped / fused launches (as the call saw them at its start)
  const bool use_group = p.opt.mrf_group, use_pair = h.resblock_type == 1 && use_group && p.opt.rb_pair;
  for (int d = 0; d < nd; ++d) {
    HPlan c1[3], c2[3];
    HPairPlan pp[3];
    uint4* dst[3];
    for (int j = 0; j < nk; ++j) {
      const HResConv& rc = p.hm->h_rb[st.i][j][d];
      const int K = h.resblock_kernel_sizes[j], dil = h.resblock_dilations[j][d];
      const double flop = 2.0 * ch * ch * K * (double)Lout * B;
      dst[j] = step_dst(pl[j], d, nd);
      if (h.resblock_type == 1) {
        // ResBlock1.forward (models.py:91-98): xt = c2(lrelu(c1(lrelu(x)))); x = xt + x.  conv1 stores lrelu(c1(.)) — its only
        // consumer is conv2, which would apply it on load
        HConvArgs a1 = f16_conv_args(p, plane(rin[j]), plane(pl[j].t), dil, (K * dil - dil) / 2);
        HConvArgs a2 = f16_conv_args(p, plane(pl[j].t), plane(dst[j]), 1, (K - 1) / 2);
        a1.in_slope = a1.out_slope = 0.1f;
        a2.res = rin[j];
        c1[j] = plan_f16(rc.c1, a1, EPI_LINEAR, B, Lout, flop);
        c2[j] = plan_f16(rc.c2, a2, EPI_LINEAR, B, Lout, flop);
        pp[j].a = f16_pair_args(p, st, rc, rin[j], dst[j], dil);
        pp[j].K = K;
        pp[j].flop = 2.0 * flop;
      } else {
        // ResBlock2.forward (models.py:136-141): x = c(lrelu(x)) + x
        HConvArgs a = f16_conv_args(p, plane(rin[j]), plane(dst[j]), dil, (K * dil - dil) / 2);
        a.in_slope = 0.1f;
        a.res = rin[j];
        c1[j] = plan_f16(rc.c1, a, EPI_LINEAR, B, Lout, flop);
      }
    }
    int fused = 1;
    if (use_pair) {
      fused = run_pair_group_f16(p.ctx, p.w, pp, nk, ch, B, Lout, p.s);
      if (fused < 0) return fused;
      if (fused == 0 && p.taps)
        for (int j = 0; j < nk; ++j) CHECK(voc_tap(p, tap_name("rb%d.%d.%d", st.i, j, d), dst[j], true, ch, st.ldo, st.mul));
    }
    for (int pass = 0; fused != 0 && pass < (h.resblock_type == 1 ? 2 : 1); ++pass) {
      const HPlan* plans = pass ? c2 : c1;
      int rc = use_group ? run_group_f16(p.ctx, p.w, plans, nk, B, p.s) : 1;
      if (rc < 0) return rc;
      if (rc == 1)
        for (int j = 0; j < nk; ++j) CHECK(run_plan_f16(p.ctx, p.w, plans[j], KC_RESBLOCK, p.s));
      if (p.taps) {  // pass 0 of a ResBlock1 step leaves conv1's stored output, every other pass the step's own
        const bool t_plane = h.resblock_type == 1 && pass == 0;
        for (int j = 0; j < nk; ++j)
          CHECK(voc_tap(p, tap_name(t_plane ? "rb%d.%d.%d.t" : "rb%d.%d.%d", st.i, j, d), t_plane ? pl[j].t : dst[j], true, ch, st.ldo, st.mul));
      }
    }
    for (int j = 0; j < nk; ++j) rin[j] = dst[j];
  }
  uint4* outs[3] = {nullptr, nullptr, nullptr};
  for (int j = 0; j < nk; ++j) outs[j] = pl[j].dst_last;
  c.advance(st, outs, nk, (float)nk, true);
  return 0;
}

static int f16_post(VocPass& p, const StageCursor<uint4>& c) {  // x = tanh(conv_post(leaky_relu(x)))  — default slope 0.01 (models.py:198-201)
  HPostArgs a = post_args<HPostArgs>(p, c, (long long)(c.ch / 8) * c.ldin);
  a.peak = p.peak;
  a.peak_ld = p.peak_ld;
  {
    ProfScope ps(p.ctx, p.w, KC_VOC_IO, 2.0 * (double)c.ch * 7 * (double)c.Lin * p.B, p.s);
    ps.kernel(KN_POST_F16);
    const dim3 pg((c.Lin + HPOST_TW - 1) / HPOST_TW, p.B);
    switch_const<1, 2, 3>(c.ncur, [&](auto n) { hipLaunchKernelGGL(HIP_KERNEL_NAME(post_f16_kernel<7, decltype(n)::value>), pg, dim3(256), 0, p.s, a); });
  }
  if (p.taps) CHECK(voc_tap(p, "wav", p.wav, false, 1, (int)p.Nld, c.mul));
  return 0;
}

// Leaves the f32 waveform rows in `p.wav` ([B][Nld]) and, when asked, the |max| of every 256-sample tile in `p.peak`
// (voc_out.h's wave_out_kernel reads both).
static int hifigan_body_f16(VocPass& p) {
  StageCursor<uint4> c;
  CHECK(f16_pre(p, c));
  for (int i = 0; i < p.hm->hp.num_upsamples; ++i) {
    const VocStage st = voc_stage(p.hm->hp, i, c.Lin, c.mul, true);
    CHECK(f16_upsample(p, c, st));
    CHECK(f16_resblocks(p, c, st));
  }
  return f16_post(p, c);
}

// ------------------------------------------------------------------ the stages of a call behind the generator
// HiFiGanVocoder.denoise (larynx/hifi_gan.py:171-179); returns the rows the delivery reads
static float* voc_denoise(VocPass& p) {
  if (!p.denoise) return p.wav;
  ProfScope ps(p.ctx, p.w, KC_SMALL, 0);
  hipLaunchKernelGGL(stft_denoise_kernel, dim3(p.Tmax, p.B), dim3(256), 0, p.s, p.wav, (long long)p.Nld, p.d_frames, p.hop, p.bias_spec,
                     p.denoiser_strength, p.fbuf, p.Tmax, (float*)nullptr);
  hipLaunchKernelGGL(overlap_add_kernel, dim3(256, p.B), dim3(256), 0, p.s, p.fbuf, p.Tmax, p.d_frames, p.hop, p.wav2, (long long)p.Nld,
                     (long long)p.Nld);
  return p.wav2;
}

// Option "voc_out": ONE launch delivers the rows: to the caller's device buffers (pause before | samples | zeros up to the row
// stride), or to the staging buffers the host copy reads (the float rows in place: zero tails behind a short row's samples)
static int voc_tail_one_launch(VocPass& p, const VocCall& call, float* wav) {
  const bool out_dev = p.out_dev;
  const int B = p.B;
  ProfScope ps(p.ctx, p.w, KC_SMALL, 0);
  if (p.any_i16 && !p.peak) {  // behind the denoiser: one peak per row, from the denoised rows
    HIPCHECK(hipMemsetAsync(p.peaks, 0, sizeof(unsigned) * B, p.s));
    hipLaunchKernelGGL(absmax_kernel, dim3(128, B), dim3(256), 0, p.s, wav, (long long)p.Nld, p.d_frames, p.hop, p.peaks);
  }
  WaveOutArgs o;
  std::memset(&o, 0, sizeof(o));
  o.wav = wav; o.bs = (long long)p.Nld; o.frames = p.d_frames; o.hop = p.hop;
  o.peak = reinterpret_cast<const float*>(p.peaks);
  o.peak_ld = p.peak ? p.peak_ld : 1;
  o.peak_parts = p.peak ? 0 : 1;
  o.pad_before = call.pad_before;
  bool any_out = false;
  if (call.rows) {
    o.per_row = 1;
    for (int b = 0; b < B; ++b) {
      const VocRow& r = call.rows[b];
      o.pad_rows[b] = r.pad_before;
      if (out_dev) {
        o.f32_rows[b] = r.wav_f32; o.f_ld_rows[b] = r.wav_ld;
        o.i16_rows[b] = r.wav_i16; o.i_ld_rows[b] = r.wav_ld;
      } else if (r.wav_i16) {
        o.i16_rows[b] = p.i16 + (size_t)b * p.ild; o.i_ld_rows[b] = (long long)p.ild;
      }
      any_out = any_out || o.f32_rows[b] || o.i16_rows[b];
    }
  } else if (out_dev) {
    if (call.wav_f32) { o.f32 = call.wav_f32; o.f_bs = call.wav_ld; o.f_ld = call.wav_ld; }
    if (call.wav_i16) { o.i16 = call.wav_i16; o.i_bs = call.wav_ld; o.i_ld = call.wav_ld; }
  } else {
    // (the float rows stay where they are: only a short row's tail up to the longest row is zeroed, in place)
    if (call.wav_i16) { o.i16 = p.i16; o.i_bs = (long long)p.ild; o.i_ld = (long long)p.ild; }
  }
  if (o.f32 || o.i16 || any_out) {
    ps.kernel(KN_WAVE_OUT);
    hipLaunchKernelGGL(wave_out_kernel, dim3(128, B), dim3(256), 0, p.s, o);
  }
  if (!out_dev && p.any_f32 && B > 1) hipLaunchKernelGGL(zero_tail_kernel, dim3(64, B), dim3(256), 0, p.s, wav, (long long)p.Nld, (long long)p.Nld, p.d_frames, p.hop);
  return 0;
}
// "voc_out" = 0 (whole-batch destinations only): zero_tail, absmax and to_int16 into the staging rows
static int voc_tail_by_pieces(VocPass& p, const VocCall& call, float* wav) {
  ProfScope ps(p.ctx, p.w, KC_SMALL, 0);
  const int B = p.B;
  hipLaunchKernelGGL(zero_tail_kernel, dim3(64, B), dim3(256), 0, p.s, wav, (long long)p.Nld, (long long)p.Nld, p.d_frames, p.hop);
  if (call.wav_i16) {
    HIPCHECK(hipMemsetAsync(p.peaks, 0, sizeof(unsigned) * B, p.s));
    hipLaunchKernelGGL(absmax_kernel, dim3(128, B), dim3(256), 0, p.s, wav, (long long)p.Nld, p.d_frames, p.hop, p.peaks);
    hipLaunchKernelGGL(to_int16_kernel, dim3(128, B), dim3(256), 0, p.s, wav, (long long)p.Nld, p.d_frames, p.hop, p.peaks, p.i16,
                       (long long)p.ild, (long long)p.ild, call.pad_before);
  }
  return 0;
}

// The finished rows `wav` to the caller; ends with the stream synchronised
static int voc_deliver(VocPass& p, const VocCall& call, const OutRows& rows, float* wav) {
  const WavRows dev = {wav, p.Nld, p.i16, p.ild};
  if (p.voc_out) {
    CHECK(voc_tail_one_launch(p, call, wav));
  } else {
    CHECK(voc_tail_by_pieces(p, call, wav));
    if (p.out_dev) CHECK(scatter_rows(rows, p.B, dev, RowWriter{true, p.s}));
  }
  return p.out_dev ? p.frame.finish() : deliver_rows(p.frame, rows, p.B, dev, p.staged, false);
}

// The forward pass proper on frame `f` (already checked by hifigan_precheck); ends with the stream synchronised and the outputs
// delivered.  An error return behind queued kernels — possibly on the side streams — is drained by the frame.
static int hifigan_run(CallFrame& f, HifiModel* hm, const mi355tts_mel* mel, const VocCall& call) {
  const OutRows rows = call_rows(call, mel, hm->hop);
  if (mel->max_frames == 0) return zero_outputs(f, rows, mel->B, (call.flags & MI355TTS_OUT_DEVICE) != 0);
  long long sum = 0;  // profiled FLOP of a ragged batch count the rows' real frames, not B x the longest row
  for (int b = 0; b < mel->B; ++b) sum += mel->frames[b];
  f.w->flop_scale = (double)sum / ((double)mel->B * mel->max_frames);
  VocPass p(f, hm, mel, call);
  CHECK(p.bind(call, rows));
  TapNames kn_out(f.w, p.taps);
  CHECK(p.f16 ? hifigan_body_f16(p) : hifigan_body_f32(p));
  return voc_deliver(p, call, rows, voc_denoise(p));
}


// One vocoder call on a pinned model and a worker of its own; `call.precision` >= 0: the precision is already fixed
static int hifigan_call_on(mi355tts_ctx* ctx, HifiModel* hm, int vocoder, const mi355tts_mel* mel, VocCall call) {
  CHECK(hifigan_precheck(ctx, hm, vocoder, mel->frames.data(), mel->B, mel->M, mel->max_frames, call));
  CallFrame f(ctx);
  CHECK(f.open());
  return hifigan_run(f, hm, mel, call);
}

// The denoiser's bias spectrum of the generator of `precision` (the model keeps one per generator), computed on first use
static int ensure_denoiser_bias(mi355tts_ctx* ctx, HifiModel* hm, int vocoder, int precision) {
  std::lock_guard<std::mutex> lk(hm->bias_mu);
  const int bi = precision == MI355TTS_PRECISION_F16 ? 1 : 0;
  if (hm->bias_ready[bi]) return 0;
  const int M = hm->hp.num_mels, hop = hm->hop;
  const int zf = 88;  // the reference's all-zero mel has 88 frames (hifi_gan.py:187,198)
  const long long N = (long long)zf * hop;
  if (N <= DN_FFT) return fail(MI355TTS_ERR_INVALID, "vocoder hop %d too small for the 1024-point denoiser STFT", hop);
  HIPCHECK(hipSetDevice(ctx->device));
  std::vector<float> zeros((size_t)M * zf, 0.f);
  int32_t fr = zf;
  mi355tts_mel* zm = nullptr;
  CHECK(mi355tts_mel_from_buffer(ctx, zeros.data(), &fr, 1, M, zf, nullptr, 0, &zm));
  float* dwav = nullptr;
  float* bias = nullptr;
  int rc = 0;
  if (hipMalloc(&dwav, sizeof(float) * (size_t)N) != hipSuccess || hipMalloc(&bias, sizeof(float) * (DN_FFT / 2 + 1)) != hipSuccess)
    rc = fail(MI355TTS_ERR_NOMEM, "hipMalloc denoiser bias");
  if (!rc) {
    VocCall c;
    c.wav_f32 = dwav;
    c.wav_ld = N;
    c.flags = MI355TTS_OUT_DEVICE;
    c.precision = precision;
    rc = hifigan_call_on(ctx, hm, vocoder, zm, c);
  }
  if (!rc) {
    CallFrame f(ctx);
    rc = f.open();
    if (!rc) {
      hipLaunchKernelGGL(stft_denoise_kernel, dim3(1, 1), dim3(256), 0, f.s, dwav, (long long)N, zm->frames_dev, hop,
                         (const float*)nullptr, 0.f, (float*)nullptr, 1, bias);
      if (f.wait() != hipSuccess) rc = fail(MI355TTS_ERR_HIP, "denoiser bias kernel failed");
    }
  }
  mel_destroy(zm);
  if (dwav) hipFree(dwav);
  if (rc) {
    if (bias) hipFree(bias);
    return rc;
  }
  hm->bias_spec[bi] = bias;
  hm->bias_ready[bi] = true;
  return 0;
}

static int hifigan_call(mi355tts_ctx* ctx, int vocoder, const mi355tts_mel* mel, const VocCall& call) {
  if (!ctx || !mel) return fail(MI355TTS_ERR_INVALID, "null argument");
  std::shared_ptr<HifiModel> vpin;
  CHECK(find_model(ctx, vocoder, &vpin));
  return hifigan_call_on(ctx, vpin.get(), vocoder, mel, call);
}

extern "C" int mi355tts_hifigan_infer_padded(mi355tts_ctx* ctx, int vocoder, const mi355tts_mel* mel, float denoiser_strength,
                                             float* wav_f32, int16_t* wav_i16, int64_t wav_ld, uint32_t flags,
                                             int32_t pad_before, int32_t pad_after) {
  VocCall c;
  c.denoiser_strength = denoiser_strength;
  c.wav_f32 = wav_f32;
  c.wav_i16 = wav_i16;
  c.wav_ld = wav_ld;
  c.flags = flags;
  c.pad_before = pad_before;
  c.pad_after = pad_after;
  return hifigan_call(ctx, vocoder, mel, c);
}

// ------------------------------------------------------------------ the test seam's entry point (the store and the read-out: host_taps.h)
extern "C" int mi355tts_hifigan_infer_taps(mi355tts_ctx* ctx, int vocoder, const mi355tts_mel* mel, float* wav_f32, int64_t wav_ld,
                                           char* json, int cap) {
  if (!ctx || !mel || !wav_f32 || !json) return fail(MI355TTS_ERR_INVALID, "null argument");
  auto taps = std::make_shared<VocTaps>();
  VocCall c;
  c.wav_f32 = wav_f32;
  c.wav_ld = wav_ld;
  c.taps = taps.get();
  CHECK(hifigan_call(ctx, vocoder, mel, c));  // (ends with the stream synchronised: the copies are complete)
  return finish_taps(ctx, taps, json, cap);
}

extern "C" int mi355tts_hifigan_infer(mi355tts_ctx* ctx, int vocoder, const mi355tts_mel* mel, float denoiser_strength,
                                      float* wav_f32, int16_t* wav_i16, int64_t wav_ld, uint32_t flags) {
  return mi355tts_hifigan_infer_padded(ctx, vocoder, mel, denoiser_strength, wav_f32, wav_i16, wav_ld, flags, 0, 0);
}
