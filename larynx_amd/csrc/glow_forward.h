// mi355tts host runtime — mi355tts_glow_infer: the GlowTTS layer schedule (glow_tts/models.py:118-140, :191-209, :308-354)
// (one translation unit: included once by mi355tts.hip, after the kernel headers)
// GlowPass (what a run of launches shares; the launch helpers are its members), the call struct, the workspace layouts and their
// views, the fused launches, then the stages of a pass — encoder, durations, decoder (a function per flow block) — and glow_run.
// The entry points open a CallFrame and pin their model with find_model (host_call.h).
#pragma once

// ------------------------------------------------------------------ GlowTTS forward
static bool glow_fuse_on(const Worker* w) { return !w->opt.env.glow_fuse_off && w->opt.glow_fuse; }

// What is constant over a run of GlowTTS launches; one instance serves the encoder, one the decoder.  A launch helper then
// takes only what differs per launch: the conv, its ConvArgs, the norm's parameters.
struct GlowPass {
  mi355tts_ctx* ctx;
  Worker* w;
  const GlowModel* gm;
  const float* A;  // gm->arena
  hipStream_t s;
  int B, n_max, ld;  // rows, the longest row (Pmax / F2max), the row stride of every activation
  const int* d_len;  // device, [B]
  int host_len;      // the row's length at batch 1, else -1
  int glow_tiles;    // workgroup target per conv launch (tile-shape choice; tuning knob MI355TTS_GLOW_TILES)
  // every launch on the smallest tile whatever the batch size, so that a row of a coalesced pass would be computed by exactly
  // the launches of its own batch-1 call.  No caller sets it (profiles/NOTES.md, open items).
  bool solo_tiles;
  int cls;  // profile class: KC_GLOW_ENC_CONV / KC_GLOW_DEC_CONV
  // the test seam (mi355tts_glow_infer_taps): where a copy of every plane this pass writes is kept, and the rows' valid columns on
  // the host [B]; null in every other call
  VocTaps* taps = nullptr;
  const int* tap_len = nullptr;

  // A copy of the f32 plane `x` [B][ch][ld], queued right behind the launch that wrote it (the passes rewrite their planes in
  // place; host_taps.h).  `same_launch`: the second plane of the launch that wrote the previous tap.  Callers test `taps` first.
  int tap(const std::string& name, const float* x, int ch, bool same_launch = false) const {
    return taps->add(s, name, x, false, B, ch, ld, tap_len, same_launch);
  }

  RowLen rows() const { return row_len(B, host_len, d_len); }
  ProfScope small() const { return ProfScope(ctx, w, KC_SMALL, 0); }
  // a conv over this pass's activations: x [B][.][ld] -> y [B][.][ld]
  ConvArgs args(const float* x, long long x_bs, float* y, long long y_bs, int dil = 1, int pad = 0) const {
    return base_args(x, x_bs, ld, d_len, 1, y, y_bs, ld, d_len, 1, dil, pad);
  }
  int conv(const DevConv& c, const ConvArgs& a, int epi = EPI_LINEAR) const {
    return launch_conv(ctx, w, c, a, epi, B, n_max, cls, nullptr, glow_tiles, host_len);
  }
  int lin16(const DevConv& c, const ConvArgs& a, const Lin16Ln* ln = nullptr) const {
    return run_lin16(ctx, w, c, a, A, B, n_max, cls, host_len, solo_tiles, ln);
  }
  int gate16(const DevConv& c, const ConvArgs& a) const { return run_gate16(ctx, w, c, a, B, n_max, cls, s); }

  void layernorm(const float* x, const float* g, const float* b, float* y, int C, long long bs, int post_relu) const {
    ProfScope ps = small();
    const float* res = nullptr;
    if (C <= 256)
      hipLaunchKernelGGL(layernorm16_kernel, dim3((n_max + 15) / 16, B), dim3(256), 0, s, x, res, g, b, y, C, bs, ld, d_len, 0, post_relu,
                         1e-4f);
    else
      hipLaunchKernelGGL(layernorm_kernel, dim3((n_max + 63) / 64, B), dim3(256), 0, s, x, res, g, b, y, C, bs, ld, d_len, 0, post_relu,
                         1e-4f);
  }
  // an encoder conv: the 16-row tile with the input staged once when the shape has one (lin16_kernel), else the generic tile
  int enc_conv(const DevConv& c, const ConvArgs& a) const {
    if (lin16(c, a) == 0) return 0;
    return conv(c, a);
  }
  // LayerNorm -> [ReLU] -> conv with the norm inside the conv launch (lin16_kernel's LN prologue) when the shape has one;
  // otherwise the LayerNorm launch (raw -> normed) and the conv on its output.  a.x is the raw tensor; ln.out (where the
  // normalised tensor is also stored) may be nullptr when nothing else reads it AND the fused form is taken; the fallback needs
  // a buffer: `scratch`.
  // Taps: the conv's output under the name `fmt` gives with `idx`, the stored normalised tensor under `ln_fmt`'s — in the fallback
  // the LayerNorm launch's output, that name + ".ln" where ln.out is null.  (The names are built only where `taps` is set.)
  int ln_conv(const DevConv& c, ConvArgs a, const Lin16Ln& ln, float* scratch, const char* fmt, int idx = 0, const char* ln_fmt = nullptr) const {
    if (!w->opt.env.lin16_no_ln && glow_fuse_on(w) && lin16(c, a, &ln) == 0) {
      if (taps) {
        CHECK(tap(tap_name(fmt, idx), a.y, c.Cout));
        if (ln.out) CHECK(tap(tap_name(ln_fmt, idx), ln.out, c.Cin, true));
      }
      return 0;
    }
    float* dst = ln.out ? ln.out : scratch;
    layernorm(a.x, ln.gamma, ln.beta, dst, c.Cin, a.x_bs, ln.relu);
    if (taps) CHECK(tap(ln.out ? tap_name(ln_fmt, idx) : tap_name(fmt, idx) + ".ln", dst, c.Cin));
    a.x = dst;
    CHECK(enc_conv(c, a));
    return taps ? tap(tap_name(fmt, idx), a.y, c.Cout) : 0;
  }
};

struct GlowCall {
  const int64_t* ids = nullptr;
  const int32_t* id_lens = nullptr;
  int B = 0, ids_ld = 0;
  float noise_scale = 0.667f, length_scale = 1.0f;
  const float* noise = nullptr;
  int noise_ld = 0;
  uint64_t seed = 0;
  const uint64_t* row_seeds = nullptr;  // optional, host, [B]: the noise stream of row b (default seed + b)
  const int32_t* speaker_ids = nullptr;  // host, [B]: multi-speaker voices only (required there, forbidden otherwise)
  // optional, host, [B]: row b's ids live at row_ids[b] (id_lens[b] of them; host or device per `flags`) instead of
  // ids + b * ids_ld — the rows of a coalesced pass come from different callers (host_join.h)
  const int64_t* const* row_ids = nullptr;
  // every launch on the smallest tile whatever the batch size: what a batch-1 call uses up to ~5000 decoder columns, so
  // a row of a coalesced pass would be computed by exactly the launches (and summation orders) of its own batch-1 call
  // (GlowPass::solo_tiles; no caller sets it)
  bool solo_tiles = false;
  const mi355tts_audio_settings* audio = nullptr;
  uint32_t flags = 0;
  // prosody (mi355tts_prosody), all host [B][pros_ld] like speaker_ids: a rate per id, or durations that stand in for the
  // predictor's; want_durations: the mel keeps what every id got (durations_out, when given, receives a copy)
  const float* id_scales = nullptr;
  const int32_t* durations_in = nullptr;
  int32_t* durations_out = nullptr;
  int pros_ld = 0;
  bool want_durations = false;
  void set_prosody(const mi355tts_prosody* p, bool keep) {
    if (!p) return;
    id_scales = p->id_scales;
    durations_in = p->durations_in;
    durations_out = p->durations_out;
    pros_ld = p->ld;
    want_durations = keep || p->durations_out;
  }
  bool has_prosody() const { return id_scales || durations_in || want_durations; }
  VocTaps* taps = nullptr;  // mi355tts_glow_infer_taps: keep a copy of every plane the schedule writes (GlowPass::tap); else null
};

static int glow_precheck(const GlowModel* gm, const GlowCall& c, int* Pmax_out) {
  if ((!c.ids && !c.row_ids) || !c.id_lens) return fail(MI355TTS_ERR_INVALID, "null argument");
  if (c.B <= 0 || c.ids_ld <= 0) return fail(MI355TTS_ERR_INVALID, "empty batch");
  // the reference fails on either mismatch (no emb_g to index / a duration predictor built for hidden + gin channels)
  if (gm->gin() && !c.speaker_ids)
    return fail(MI355TTS_ERR_INVALID, "this voice has %d speakers: pass speaker ids (mi355tts_glow_infer_speakers / mi355tts_synthesize_speakers)",
                gm->hp.n_speakers);
  if (!gm->gin() && c.speaker_ids) return fail(MI355TTS_ERR_INVALID, "speaker ids given to a single-speaker voice");
  if (c.speaker_ids)
    for (int b = 0; b < c.B; ++b)
      if (c.speaker_ids[b] < 0 || c.speaker_ids[b] >= gm->hp.n_speakers)  // nn.Embedding raises on an out-of-range index
        return fail(MI355TTS_ERR_INVALID, "speaker_ids[%d]=%d outside [0,%d)", b, c.speaker_ids[b], gm->hp.n_speakers);
  int Pmax = 0;
  for (int b = 0; b < c.B; ++b) {
    if (c.id_lens[b] < 1 || c.id_lens[b] > c.ids_ld)
      return fail(MI355TTS_ERR_INVALID, "id_lens[%d]=%d outside [1,%d]", b, c.id_lens[b], c.ids_ld);
    Pmax = std::max(Pmax, c.id_lens[b]);
  }
  if (!(c.flags & MI355TTS_IN_DEVICE)) {
    // the reference's embedding lookup raises on an out-of-range id (glow_tts/models.py:119);
    // device-resident ids cannot be checked without a sync and are clamped by the kernel instead
    for (int b = 0; b < c.B; ++b)
      for (int t = 0; t < c.id_lens[b]; ++t) {
        const int64_t id = c.row_ids ? c.row_ids[b][t] : c.ids[(size_t)b * c.ids_ld + t];
        if (id < 0 || id >= gm->hp.num_symbols)
          return fail(MI355TTS_ERR_INVALID, "phoneme id %lld at [%d][%d] outside [0,%d)", (long long)id, b, t, gm->hp.num_symbols);
      }
  }
  if (c.has_prosody()) {
    if (c.id_scales && c.durations_in) return fail(MI355TTS_ERR_INVALID, "prosody: id_scales and durations_in exclude each other");
    for (int b = 0; b < c.B; ++b) {
      if (c.pros_ld < c.id_lens[b])
        return fail(MI355TTS_ERR_INVALID, "prosody: ld %d < id_lens[%d]=%d", c.pros_ld, b, c.id_lens[b]);
      for (int t = 0; t < c.id_lens[b]; ++t) {
        const size_t i = (size_t)b * c.pros_ld + t;
        if (c.id_scales && !(std::isfinite(c.id_scales[i]) && c.id_scales[i] >= 0.f))
          return fail(MI355TTS_ERR_INVALID, "prosody: id_scales[%d][%d]=%g is not a finite value >= 0", b, t, (double)c.id_scales[i]);
        if (c.durations_in && (c.durations_in[i] < 0 || c.durations_in[i] > (1 << 28)))
          return fail(MI355TTS_ERR_INVALID, "prosody: durations_in[%d][%d]=%d outside [0, 2^28]", b, t, c.durations_in[i]);
      }
    }
  }
  *Pmax_out = Pmax;
  return 0;
}

// Encoder workspace of one call: ONE definition for the forward pass and mi355tts_reserve.
struct GlowEncLayout {
  size_t o_len, o_seed, o_ids, o_x, o_t1, o_t2, o_qkv, o_ffn, o_xm, o_logw, o_cum, o_sc, o_spk, o_cond, o_dps, total;
  // a call's id_scales or durations_in (one of them, 4-byte entries, row stride P) sit right behind the region, where the decoder's
  // workspace is appended later: duration_kernel has consumed them by then.  Not part of `total`: no other call's layout changes.
  size_t o_pros, pros_end;
  int P, att_rows;
};
static GlowEncLayout glow_enc_layout(const mi355tts_glow_hparams& h, int B, int ids_ld, int Pmax) {
  GlowEncLayout L;
  const int H = h.hidden_channels, Fc = h.filter_channels, Fd = h.filter_channels_dp, M = h.mel_channels;
  L.P = (Pmax + 3) & ~3;
  const int P = L.P;
  Carver cv;
  L.o_len = cv.take(sizeof(int) * B);
  L.o_seed = cv.take(sizeof(unsigned long long) * B);
  L.o_ids = cv.take(sizeof(long long) * (size_t)B * ids_ld);
  L.o_x = cv.take(sizeof(float) * (size_t)B * H * P);
  L.o_t1 = cv.take(sizeof(float) * (size_t)B * H * P);
  L.o_t2 = cv.take(sizeof(float) * (size_t)B * H * P);
  L.o_qkv = cv.take(sizeof(float) * (size_t)B * 3 * H * P);
  L.o_ffn = cv.take(sizeof(float) * (size_t)B * std::max(Fc, 3 * Fd) * P);
  L.o_xm = cv.take(sizeof(float) * (size_t)B * M * P);
  L.o_logw = cv.take(sizeof(float) * (size_t)B * P);
  L.o_cum = cv.take(sizeof(int) * (size_t)B * P);
  L.att_rows = ((Pmax + ATT_ROWS - 1) / ATT_ROWS) * ATT_ROWS;
  // score scratch: only the VALU attention fallback (P > ATTM_MAXP) uses it
  L.o_sc = cv.take(Pmax > ATTM_MAXP ? sizeof(float) * (size_t)B * h.n_heads * L.att_rows * P : 0);
  // multi-speaker voices: speaker ids, the decoder's gate offsets [B][n_blocks][2H n_layers] (live until the last flow block:
  // the encoder region is kept when the decoder's is appended) and the duration predictor's per-tap speaker sums [B][Fd][k]
  const bool spk = h.n_speakers > 1;
  L.o_spk = cv.take(spk ? sizeof(int) * B : 0);
  L.o_cond = cv.take(spk ? sizeof(float) * (size_t)B * h.n_blocks_dec * 2 * H * h.n_block_layers : 0);
  L.o_dps = cv.take(spk ? sizeof(float) * (size_t)B * Fd * h.kernel_size : 0);
  L.total = cv.pos;
  L.o_pros = cv.take(0);
  L.pros_end = L.o_pros + sizeof(float) * (size_t)B * P;
  return L;
}
struct GlowDecLayout {
  size_t o_z, o_h, o_ac, o_sk, o_nz, total;
};
static GlowDecLayout glow_dec_layout(const mi355tts_glow_hparams& h, size_t enc_bytes, int B, int Fmax, size_t host_noise_floats) {
  GlowDecLayout L;
  const int H = h.hidden_channels, C = h.mel_channels * h.n_sqz;
  const int F2 = (Fmax / h.n_sqz + 3) & ~3;
  Carver dv;
  dv.pos = enc_bytes;
  L.o_z = dv.take(sizeof(float) * (size_t)B * C * F2);
  L.o_h = dv.take(sizeof(float) * (size_t)B * H * F2);
  L.o_ac = dv.take(sizeof(float) * (size_t)B * H * F2);
  L.o_sk = dv.take(sizeof(float) * (size_t)B * H * F2);
  L.o_nz = dv.take(sizeof(float) * host_noise_floats);
  L.total = dv.pos;
  return L;
}

// The layouts bound to an arena: EVERY buffer, so that a pass which re-binds after the arena moved cannot miss one.
struct GlowEncView {
  int* len;
  unsigned long long* seeds;
  long long* ids;
  float *x, *t1, *t2, *qkv, *ffn, *xm, *logw;
  int* cum;
  float* sc;
  int* spk;
  float *cond, *dps;
  void* pros;
};
static GlowEncView glow_enc_view(const GlowEncLayout& L, char* base) {
  auto f = [&](size_t off) { return (float*)(base + off); };
  auto i = [&](size_t off) { return (int*)(base + off); };
  return {i(L.o_len), (unsigned long long*)(base + L.o_seed), (long long*)(base + L.o_ids), f(L.o_x), f(L.o_t1), f(L.o_t2), f(L.o_qkv), f(L.o_ffn),
          f(L.o_xm), f(L.o_logw), i(L.o_cum), f(L.o_sc), i(L.o_spk), f(L.o_cond), f(L.o_dps), base + L.o_pros};
}
struct GlowDecView {
  float *z, *h, *acts, *skip, *nz;
};
static GlowDecView glow_dec_view(const GlowDecLayout& L, char* base) {
  auto f = [&](size_t off) { return (float*)(base + off); };
  return {f(L.o_z), f(L.o_h), f(L.o_ac), f(L.o_sk), f(L.o_nz)};
}

// One forward pass on worker `w`: what its stages share.
struct GlowRun {
  mi355tts_ctx* ctx;
  Worker* w;
  const GlowModel* gm;
  const GlowCall& call;
  int Pmax;
  int glow_tiles;
  GlowEncLayout el;
  GlowEncView ev;
  mi355tts_mel* mel;
  GlowPass pass(int n_max, int ld, const int* d_len, int host_len, int cls, const int* tap_len = nullptr) const {
    return {ctx, w, gm, gm->arena, w->stream, call.B, n_max, ld, d_len, host_len, glow_tiles, call.solo_tiles, cls, call.taps, tap_len};
  }
};

// ---- column-owner launches (coltile.h).  Each returns 1 when the shape is not one the kernel takes (the caller then runs
// the separate launches), 0 when launched.
// conv_o + residual + LayerNorm of encoder layer `L`: x = LayerNorm(x + conv_o(att))
static int run_oproj_ln(const GlowPass& p, const GlowLayer& L, const float* att, float* x) {
  const int H = p.gm->hp.hidden_channels;
  if (!glow_fuse_on(p.w) || !L.o16.ok || H > COL_MAXROWS || p.ld % 4 || p.n_max <= 0) return 1;
  OprojLnArgs a;
  std::memset(&a, 0, sizeof(a));
  a.x = att; a.res = x; a.y = x; a.bs = (long long)H * p.ld; a.ld = p.ld;
  p.rows().into(a);
  a.len_mul = 1;
  a.w = p.A + L.o16.w_off; a.b = p.A + L.o16.b_off; a.gamma = p.A + L.g1; a.beta = p.A + L.b1;
  a.H = H; a.eps = 1e-4f;
  ProfScope ps(p.ctx, p.w, p.cls, 2.0 * (double)H * H * (double)p.n_max * p.B);
  ps.kernel(KN_OPROJ_LN);
  hipLaunchKernelGGL(oproj_ln_kernel, dim3((p.n_max + COL_T - 1) / COL_T, p.B), dim3(512), 0, p.s, a);
  return 0;
}
// the tail of block `Bk` and the start of `next` (nullptr after the last block in reverse order)
static int run_glow_tail(const GlowPass& p, const GlowDecView& dv, const GlowBlock& Bk, const GlowBlock* next) {
  const mi355tts_glow_hparams& h = p.gm->hp;
  const int H = h.hidden_channels, half = h.mel_channels * h.n_sqz / 2, F2 = p.ld;
  if (!glow_fuse_on(p.w) || !Bk.t_rs.ok || !Bk.t_end.ok || !Bk.t_st.ok || (next && !next->t_st.ok) || h.n_split != 4 || (half % 2) || F2 % 4 ||
      p.n_max <= 0)
    return 1;
  const float* A = p.A;
  GlowTailArgs a;
  std::memset(&a, 0, sizeof(a));
  a.acts = dv.acts; a.skip = h.n_block_layers > 1 ? dv.skip : nullptr; a.hnext = next ? dv.h : nullptr; a.h_bs = (long long)H * F2; a.h_ld = F2;
  a.z = dv.z; a.z_bs = (long long)h.mel_channels * h.n_sqz * F2; a.z_ld = F2;
  p.rows().into(a);
  a.len_mul = 1;
  a.w_rs = A + Bk.t_rs.w_off; a.b_rs = A + Bk.t_rs.b_off;
  a.w_end = A + Bk.t_end.w_off; a.b_end = A + Bk.t_end.b_off;
  const GlowBlock& stb = next ? *next : Bk;  // the last block has no successor: its own start stands in (loaded, never used)
  a.w_st = A + stb.t_st.w_off; a.b_st = A + stb.t_st.b_off;
  a.mix_w = A + Bk.winv; a.mix_bias = A + Bk.an_bias; a.mix_scale = A + Bk.an_scale;
  a.H = H; a.half = half;
  const double mac = (double)H * H + 2.0 * half * H + (next ? (double)H * half : 0.0);
  ProfScope ps(p.ctx, p.w, p.cls, 2.0 * mac * (double)p.n_max * p.B);
  ps.kernel(KN_GLOW_TAIL);
  hipLaunchKernelGGL(glow_tail_kernel, dim3((p.n_max + COL_T - 1) / COL_T, p.B), dim3(512), 0, p.s, a);
  return 0;
}

// the fp16 mode's WaveNet of block `Bk` (wn_f16.h): every layer's gate conv and res_skip but the last res_skip in ONE launch;
// leaves `acts` (last layer's gated activations) and `skip` (layers 0 .. n - 2) as the f32 chain would.  1 = not taken.
static int run_wn_f16(const GlowPass& p, const GlowDecView& dv, const GlowBlock& Bk) {
  const mi355tts_glow_hparams& h = p.gm->hp;
  const int H = h.hidden_channels, n = h.n_block_layers;
  if (!p.gm->f16_ok || (int)Bk.h_in.size() != n || (int)Bk.h_rs.size() != n - 1 || p.n_max <= 0 || (H != 192 && H != 32)) return 1;
  WnF16Args a;
  std::memset(&a, 0, sizeof(a));
  a.h = dv.h; a.bs = (long long)H * p.ld; a.ld = p.ld;
  p.rows().into(a);
  for (int j = 0; j < n; ++j) {
    a.w_in[j] = Bk.h_in[j].w; a.b_in[j] = Bk.h_in[j].bias;
    if (j < n - 1) { a.w_rs[j] = Bk.h_rs[j].w; a.b_rs[j] = Bk.h_rs[j].bias; }
  }
  a.n_layers = n;
  a.margin = (h.kernel_size_dec - 1) / 2 * n;
  a.acts = dv.acts; a.skip = dv.skip;
  const int to = WN_W - 2 * a.margin;
  const dim3 grid((p.n_max + to - 1) / to, p.B);
  const double mac = (double)n * 2.0 * H * H * h.kernel_size_dec + (double)(n - 1) * 2.0 * H * H;
  ProfScope ps(p.ctx, p.w, p.cls, 2.0 * mac * (double)p.n_max * p.B);
  // MI355TTS_WN_REPEAT (probe): the launch N times — it is idempotent; run 2 .. N find the block's weights in L2
  const int repeat = std::max(1, p.w->opt.env.wn_repeat);
  for (int r = 0; r < repeat; ++r) {
    if (H == 192)
      hipLaunchKernelGGL((wn_f16_kernel<5, 24, 3, 10>), grid, dim3(256), 0, p.s, a);
    else
      hipLaunchKernelGGL((wn_f16_kernel<5, 4, 1, 6>), grid, dim3(256), 0, p.s, a);
  }
  ps.kernel(KN_WN_F16);
  return 0;
}

// relative-position attention of layer `L`: qkv -> t2.  The MFMA kernel by head width (NK k-steps, EXACT when they cover it
// without padding) and by row length (the 256-id LDS layout, or the ATTM_MAXP one); past ATTM_MAXP ids the VALU kernel.
static void launch_attention(const GlowPass& p, const GlowLayer& L, const GlowEncView& v, int att_rows) {
  const mi355tts_glow_hparams& h = p.gm->hp;
  const int H = h.hidden_channels, nh = h.n_heads, P = p.ld, Pmax = p.n_max;
  const long long bsH = (long long)H * P;
  ProfScope ps = p.small();
  if (Pmax > ATTM_MAXP) {
    ps.kernel(KN_ATTENTION_VALU);
    hipLaunchKernelGGL(attention_kernel, dim3(att_rows / ATT_ROWS, nh, p.B), dim3(256), 0, p.s, v.qkv, 3 * bsH, P, p.d_len, H, nh,
                       h.window_size, p.A + L.ek, p.A + L.ev, v.t2, bsH, P, v.sc, P);
    return;
  }
  const dim3 ag((Pmax + 31) / 32, nh, p.B);
  const int dkh = H / nh;
  const int nk = dkh <= 32 ? 16 : dkh <= 64 ? 32 : dkh <= 96 ? 48 : 64;
  const bool small_lds = Pmax <= 256 && !p.w->opt.env.att_big_lds;  // (A/B runs)
  ps.kernel(small_lds ? KN_ATTENTION : KN_ATTENTION_P768);
  auto launch = [&](auto k, auto exact, auto pm) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(attention_mfma_kernel<decltype(k)::value, decltype(exact)::value != 0, decltype(pm)::value>), ag,
                       dim3(512), 0, p.s, v.qkv, 3 * bsH, P, p.d_len, H, nh, h.window_size, p.A + L.ek, p.A + L.ev, v.t2, bsH, P);
  };
  switch_const<16, 32, 48, 64>(nk, [&](auto k) {
    switch_const<0, 1>(dkh == 2 * nk ? 1 : 0, [&](auto exact) {
      if (small_lds) launch(k, exact, int_c<256>{});
      else launch(k, exact, int_c<ATTM_MAXP>{});
    });
  });
}

// ---- stage 1, the encoder (models.py:118-140): uploads, speaker conditioning, embed, prenet, attention layers, proj_m and the
// duration predictor.  Leaves x_m, logw and everything a later stage reads in r.ev.
static int glow_enc_upload(GlowRun& r) {
  const GlowCall& call = r.call;
  const mi355tts_glow_hparams& h = r.gm->hp;
  const int B = call.B, ids_ld = call.ids_ld;
  hipStream_t s = r.w->stream;
  const bool in_dev = (call.flags & MI355TTS_IN_DEVICE) != 0;
  // a call's id_scales or durations_in (one of them) sit right behind the encoder's region (GlowEncLayout::o_pros)
  const void* pros_src = call.id_scales ? (const void*)call.id_scales : (const void*)call.durations_in;
  CHECK(reserve(r.w, pros_src ? r.el.pros_end : r.el.total));
  r.ev = glow_enc_view(r.el, r.w->arena);
  const GlowEncView& v = r.ev;
  HIPCHECK(hipMemcpyAsync(v.len, call.id_lens, sizeof(int) * B, hipMemcpyHostToDevice, s));
  if (call.row_seeds) HIPCHECK(hipMemcpyAsync(v.seeds, call.row_seeds, sizeof(unsigned long long) * B, hipMemcpyHostToDevice, s));
  if (call.row_ids) {
    HIPCHECK(hipMemsetAsync(v.ids, 0, sizeof(long long) * (size_t)B * ids_ld, s));
    for (int b = 0; b < B; ++b)
      HIPCHECK(hipMemcpyAsync(v.ids + (size_t)b * ids_ld, call.row_ids[b], sizeof(long long) * (size_t)call.id_lens[b],
                              in_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  } else {
    HIPCHECK(hipMemcpyAsync(v.ids, call.ids, sizeof(long long) * (size_t)B * ids_ld, in_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  }
  // prosody inputs go up with the ids
  if (pros_src)
    HIPCHECK(hipMemcpy2DAsync(v.pros, sizeof(float) * r.el.P, pros_src, sizeof(float) * call.pros_ld, sizeof(float) * r.Pmax, (size_t)B,
                              hipMemcpyHostToDevice, s));
  // multi-speaker voices: everything the speaker vector feeds, once per call (small_kernels.h: speaker_cond_kernel)
  if (const int gin = r.gm->gin()) {
    const float* A = r.gm->arena;
    const int k = h.kernel_size, n2 = 2 * h.hidden_channels * h.n_block_layers;  // n2: gate offsets per flow block
    HIPCHECK(hipMemcpyAsync(v.spk, call.speaker_ids, sizeof(int) * B, hipMemcpyHostToDevice, s));
    ProfScope ps(r.ctx, r.w, KC_SMALL, 0);
    hipLaunchKernelGGL(speaker_cond_kernel, dim3(h.n_blocks_dec + 1, B), dim3(256), 0, s, A + r.gm->emb_g, h.n_speakers, gin, v.spk,
                       A + r.gm->cond_w, A + r.gm->cond_b, h.n_blocks_dec, n2, v.cond, A + r.gm->dp_wg, h.filter_channels_dp * k, k, v.dps);
  }
  return 0;
}

// ConvReluNorm: conv -> LayerNorm -> ReLU (x3), then x + proj(.)  (layers.py:73-80)
// Each LayerNorm -> ReLU runs inside the conv that consumes it (ln_conv): conv_0 writes its raw output, conv_i normalises
// conv_{i-1}'s, proj the last one's.  Raw outputs alternate between t1 and t2; qkv is the fallback's scratch.
static int glow_prenet(const GlowPass& p, const GlowEncView& v) {
  const GlowModel* gm = p.gm;
  const mi355tts_glow_hparams& h = gm->hp;
  const long long bsH = (long long)h.hidden_channels * p.ld;
  const int pad = h.prenet_kernel_size / 2;
  float* raw = v.t1;
  CHECK(p.enc_conv(gm->pre_conv[0], p.args(v.x, bsH, raw, bsH, 1, pad)));
  if (p.taps) CHECK(p.tap("pre.0", raw, h.hidden_channels));
  for (int i = 1; i < h.prenet_layers; ++i) {
    float* out = raw == v.t1 ? v.t2 : v.t1;
    CHECK(p.ln_conv(gm->pre_conv[i], p.args(raw, bsH, out, bsH, 1, pad), {p.A + gm->pre_g[i - 1], p.A + gm->pre_b[i - 1], 1, nullptr}, v.qkv,
                    "pre.%d", i));
    raw = out;
  }
  ConvArgs a = p.args(raw, bsH, v.x, bsH);
  a.res = v.x;
  const int last = h.prenet_layers - 1;
  return p.ln_conv(gm->pre_proj, a, {p.A + gm->pre_g[last], p.A + gm->pre_b[last], 1, nullptr}, v.qkv, "pre.proj");
}

// Encoder layer l (Encoder.forward, attentions.py:62-74).  Its norm_layers_2 rides in the next layer's qkv conv: `prev` is the
// layer whose norm is still to be applied to t1 (nullptr for the first), and the last layer applies its own.
static int glow_enc_layer(const GlowPass& p, const GlowEncView& v, int att_rows, int l) {
  const mi355tts_glow_hparams& h = p.gm->hp;
  const GlowLayer& L = p.gm->layers[l];
  const GlowLayer* prev = l > 0 ? &p.gm->layers[l - 1] : nullptr;
  const int H = h.hidden_channels, Fc = h.filter_channels, k = h.kernel_size;
  const long long bsH = (long long)H * p.ld, bsF = (long long)Fc * p.ld;
  if (prev)  // x = LayerNorm(t1) on the way in; stored too: it is the residual of this layer's conv_o and FFN
    CHECK(p.ln_conv(L.qkv, p.args(v.t1, bsH, v.qkv, 3 * bsH), {p.A + prev->g2, p.A + prev->b2, 0, v.x}, nullptr, "enc%d.qkv", l,
                    "enc%d.x0"));
  else {
    CHECK(p.enc_conv(L.qkv, p.args(v.x, bsH, v.qkv, 3 * bsH)));
    if (p.taps) CHECK(p.tap(tap_name("enc%d.qkv", l), v.qkv, 3 * H));
  }
  launch_attention(p, L, v, att_rows);
  if (p.taps) CHECK(p.tap(tap_name("enc%d.att", l), v.t2, H));
  if (run_oproj_ln(p, L, v.t2, v.x)) {
    ConvArgs a = p.args(v.t2, bsH, v.t1, bsH);
    a.res = v.x;
    CHECK(p.conv(L.o, a));
    if (p.taps) CHECK(p.tap(tap_name("enc%d.o", l), v.t1, H));
    p.layernorm(v.t1, p.A + L.g1, p.A + L.b1, v.x, H, bsH, 0);
  }
  if (p.taps) CHECK(p.tap(tap_name("enc%d.x1", l), v.x, H));
  // FFN, attentions.py:375-383
  ConvArgs a = p.args(v.x, bsH, v.ffn, bsF, 1, k / 2);
  a.out_act = ACT_RELU;
  CHECK(p.enc_conv(L.ffn1, a));
  if (p.taps) CHECK(p.tap(tap_name("enc%d.ffn", l), v.ffn, Fc));
  ConvArgs c = p.args(v.ffn, bsF, v.t1, bsH, 1, k / 2);
  c.res = v.x;
  CHECK(p.enc_conv(L.ffn2, c));
  if (p.taps) CHECK(p.tap(tap_name("enc%d.t1", l), v.t1, H));
  if (l + 1 == h.n_layers_enc) {
    p.layernorm(v.t1, p.A + L.g2, p.A + L.b2, v.x, H, bsH, 0);
    if (p.taps) CHECK(p.tap("enc.out", v.x, H));
  }
  return 0;
}

// proj_m and the duration predictor (models.py:133-139, 39-49): x -> x_m, logw
static int glow_proj_durations(const GlowPass& p, const GlowEncView& v) {
  const GlowModel* gm = p.gm;
  const mi355tts_glow_hparams& h = gm->hp;
  const float* A = p.A;
  const int H = h.hidden_channels, Fd = h.filter_channels_dp, M = h.mel_channels, k = h.kernel_size, P = p.ld, B = p.B;
  const long long bsH = (long long)H * P, bsD = (long long)Fd * P;
  CHECK(p.enc_conv(gm->proj_m, p.args(v.x, bsH, v.xm, (long long)M * P)));
  if (p.taps) CHECK(p.tap("xm", v.xm, M));
  float* d1 = v.ffn;
  float* d2 = v.ffn + (size_t)B * Fd * P;
  float* d3 = v.ffn + (size_t)2 * B * Fd * P;
  ConvArgs c1 = p.args(v.x, bsH, d1, bsD, 1, k / 2);
  c1.out_act = ACT_RELU;
  if (gm->gin()) {
    // conv_1 over [x ; g repeated along time] (models.py:128-132) = conv_1's encoder half over x + a plane that depends only
    // on the speaker and on where the row's zero padding starts: d3 is free until conv_2's fallback may use it
    {
      ProfScope ps = p.small();
      hipLaunchKernelGGL(speaker_dp_plane_kernel, dim3((P + 255) / 256, Fd, B), dim3(256), 0, p.s, v.dps, Fd, k, k / 2, p.d_len, d3, bsD, P);
    }
    c1.res = d3;
    if (p.taps) CHECK(p.tap("dp.spk", d3, Fd));
  }
  CHECK(p.enc_conv(gm->dp1, c1));
  if (p.taps) CHECK(p.tap("dp.1", d1, Fd));
  // norm_1 inside conv_2 (ln_conv): d1 -> d2; d3 is the fallback's scratch
  ConvArgs c2 = p.args(d1, bsD, d2, bsD, 1, k / 2);
  c2.out_act = ACT_RELU;
  CHECK(p.ln_conv(gm->dp2, c2, {A + gm->dg1, A + gm->db1, 0, nullptr}, d3, "dp.2"));
  if (glow_fuse_on(p.w) && Fd <= 256) {  // norm_2 and proj (1 x 1, Fd -> 1) in one launch
    {
      ProfScope ps = p.small();
      hipLaunchKernelGGL(layernorm16_kernel, dim3((p.n_max + 15) / 16, B), dim3(256), 0, p.s, d2, (const float*)nullptr, A + gm->dg2,
                         A + gm->db2, d1, Fd, bsD, P, p.d_len, 0, 0, 1e-4f, A + gm->dpp_w, A + gm->dpp_b, v.logw, (long long)P);
    }
    return p.taps ? p.tap("logw", v.logw, 1) : 0;
  }
  p.layernorm(d2, A + gm->dg2, A + gm->db2, d1, Fd, bsD, 0);
  if (p.taps) CHECK(p.tap("logw.ln", d1, Fd));
  CHECK(p.conv(gm->dpp, p.args(d1, bsD, v.logw, P)));
  return p.taps ? p.tap("logw", v.logw, 1) : 0;
}

static int glow_encoder(GlowRun& r) {
  const GlowCall& call = r.call;
  const mi355tts_glow_hparams& h = r.gm->hp;
  const int B = call.B, H = h.hidden_channels, P = r.el.P, Pmax = r.Pmax;
  long long sum = 0;
  for (int b = 0; b < B; ++b) sum += call.id_lens[b];
  r.w->flop_scale = Pmax > 0 ? (double)sum / ((double)B * Pmax) : 1.0;  // ragged batch: count the rows' real ids
  CHECK(glow_enc_upload(r));
  const GlowEncView& v = r.ev;
  const GlowPass p = r.pass(Pmax, P, v.len, B == 1 ? call.id_lens[0] : -1, KC_GLOW_ENC_CONV, call.id_lens);
  {
    ProfScope ps = p.small();
    hipLaunchKernelGGL(embed_kernel, dim3((Pmax + 63) / 64, 8, B), dim3(256), 0, p.s, v.ids, call.ids_ld, v.len, p.A + r.gm->emb,
                       h.num_symbols, H, std::sqrt((float)H), v.x, (long long)H * P, P);
  }
  if (p.taps) CHECK(p.tap("emb", v.x, H));
  if (h.prenet) CHECK(glow_prenet(p, v));
  for (int l = 0; l < h.n_layers_enc; ++l) CHECK(glow_enc_layer(p, v, r.el.att_rows, l));
  return glow_proj_durations(p, v);
}

// ---- stage 2, durations -> frame counts (the one host sync of the path): the mel object (the frame's as soon as it exists),
// duration_kernel, the read-back, the result blocks.  mel->max_frames == 0: nothing to decode.
static int glow_mel_new(mi355tts_ctx* ctx, const GlowCall& call, int M, mi355tts_mel** out) {
  const int B = call.B;
  // frames live with the result object
  auto* m = new mi355tts_mel();
  m->ctx = ctx; m->B = B; m->M = M; m->ld = 0;
  m->frames.assign(B, 0);
  m->frames_dev = (int*)pool_alloc(ctx, sizeof(int) * B);
  if (!m->frames_dev) {
    delete m;
    return fail(MI355TTS_ERR_NOMEM, "hipMalloc frames");
  }
  if (call.want_durations) {  // only a call that asks pays for the block, the copy behind the frame counts and the host vector
    m->dur_ld = call.pros_ld;
    m->dur_dev = (int*)pool_alloc(ctx, sizeof(int) * (size_t)B * m->dur_ld);
    if (!m->dur_dev) {
      mel_destroy(m);
      return fail(MI355TTS_ERR_NOMEM, "hipMalloc durations");
    }
    m->durations.assign((size_t)B * m->dur_ld, 0);
  }
  *out = m;
  return 0;
}
static int glow_durations(GlowRun& r, CallFrame& f) {
  const GlowCall& call = r.call;
  const mi355tts_glow_hparams& h = r.gm->hp;
  Worker* w = r.w;
  hipStream_t s = w->stream;
  const GlowEncView& v = r.ev;
  const int B = call.B, M = h.mel_channels, P = r.el.P;
  CHECK(glow_mel_new(r.ctx, call, M, &f.mel));
  mi355tts_mel* mel = r.mel = f.mel;
  {
    ProfScope ps(r.ctx, w, KC_SMALL, 0);
    hipLaunchKernelGGL(duration_kernel, dim3(B), dim3(64), 0, s, v.logw, (long long)P, v.len, call.length_scale, h.n_sqz, v.cum, P,
                       mel->frames_dev, 1 << 28, call.id_scales ? (const float*)v.pros : nullptr,
                       call.durations_in ? (const int*)v.pros : nullptr, P, mel->dur_dev, mel->dur_ld);
  }
  CHECK(f.pinned_ints(B));
  HIPCHECK(hipMemcpyAsync(w->pinned, mel->frames_dev, sizeof(int) * B, hipMemcpyDeviceToHost, s));
  if (mel->dur_dev)
    HIPCHECK(hipMemcpyAsync(mel->durations.data(), mel->dur_dev, sizeof(int) * mel->durations.size(), hipMemcpyDeviceToHost, s));
  HIPCHECK(mi355_sync(s));
  if (call.durations_out) std::memcpy(call.durations_out, mel->durations.data(), sizeof(int32_t) * mel->durations.size());
  int Fmax = 0;
  long long sum = 0;
  for (int b = 0; b < B; ++b) {
    mel->frames[b] = w->pinned[b];
    Fmax = std::max(Fmax, w->pinned[b]);
    sum += w->pinned[b];
  }
  if (call.noise && call.noise_scale != 0.f && call.noise_ld < Fmax)
    return fail(MI355TTS_ERR_TOO_SMALL, "noise has %d columns but the utterance needs %d frames", call.noise_ld, Fmax);
  mel->max_frames = Fmax;
  w->flop_scale = Fmax > 0 ? (double)sum / ((double)B * Fmax) : 1.0;
  mel->ld = (Fmax + 3) & ~3;
  if (Fmax == 0) return 0;
  const size_t n = (size_t)B * M * mel->ld * sizeof(float);
  mel->raw_bytes = n;
  mel->raw = (float*)pool_alloc(r.ctx, n);
  mel->voc = (float*)pool_alloc(r.ctx, n);
  if (!mel->raw || !mel->voc) return fail(MI355TTS_ERR_NOMEM, "hipMalloc mel");
  return 0;
}

// ---- stage 3, the decoder (models.py:195-206, the flows in reverse)
// The decoder's workspace is appended to the encoder's, which stays live.  When that outgrows the arena, growing moves it: the
// encoder's region goes through the host into the fresh arena and EVERY view is bound again.
static int glow_dec_workspace(GlowRun& r, const GlowDecLayout& dl, GlowDecView* dv) {
  Worker* w = r.w;
  if (dl.total > w->arena_bytes) {
    std::vector<char> keep(r.el.total);
    HIPCHECK(hipMemcpy(keep.data(), w->arena, keep.size(), hipMemcpyDeviceToHost));
    CHECK(reserve(w, dl.total));
    HIPCHECK(hipMemcpy(w->arena, keep.data(), keep.size(), hipMemcpyHostToDevice));
    r.ev = glow_enc_view(r.el, w->arena);
  }
  *dv = glow_dec_view(dl, w->arena);
  return 0;
}

// The WaveNet of a coupling block is the same function in both directions of the flow (layers.py:138-162); these two launches
// serve glow_flow_block and the forward flow of align_forward.h.
// layer j's gate conv: acts = tanh . sigmoid (in_layers[j](h) + g_l) on the 16-row gate tile, else the generic tile
static int glow_wn_gate(const GlowPass& p, const GlowDecView& dv, const float* spk_cond, int blk, int j, int dil) {
  const mi355tts_glow_hparams& h = p.gm->hp;
  const GlowBlock& Bk = p.gm->blocks[blk];
  const int H = h.hidden_channels, kd = h.kernel_size_dec, n2 = 2 * H * h.n_block_layers;  // n2: gate offsets per flow block
  const long long bsD = (long long)H * p.ld;
  ConvArgs a = p.args(dv.h, bsD, dv.acts, bsD, dil, (kd * dil - dil) / 2);
  a.half = H;
  if (spk_cond) {  // x_in + g_l (layers.py:144-154): this block's, this layer's [2H] slice of cond_layer(g), per batch row
    a.cond = spk_cond + (size_t)blk * n2 + (size_t)j * 2 * H;
    a.cond_bs = (long long)h.n_blocks_dec * n2;
  }
  // one row: the length is known on the host, no device length array to chase
  a.in_len = a.out_len = p.rows().len;
  a.in_const = a.out_const = p.rows().len_const;
  const int g16 = p.gate16(Bk.in[j], a);
  if (g16 < 0) return g16;
  if (g16 == 1) CHECK(p.conv(Bk.in[j], a, EPI_GATE));
  return p.taps ? p.tap(tap_name("blk%d.acts%d", blk, j), dv.acts, H) : 0;
}
// layer j's res_skip: h += its first half (not for the last layer, which is all skip), skip (+)= the rest
static int glow_wn_res_skip(const GlowPass& p, const GlowDecView& dv, const GlowBlock& Bk, int j, int blk = -1) {
  const int H = p.gm->hp.hidden_channels;
  const bool last = j == p.gm->hp.n_block_layers - 1;
  const long long bsD = (long long)H * p.ld;
  ConvArgs r = p.args(dv.acts, bsD, dv.h, bsD);
  r.split = last ? 0 : H;    // last layer: everything is skip
  if (!last) r.res = dv.h;  // x = x + res_skip[:H]
  r.y2 = dv.skip; r.y2_bs = bsD; r.y2_ld = p.ld; r.accum2 = j > 0;
  if (p.lin16(Bk.rs[j], r) != 0) CHECK(p.conv(Bk.rs[j], r));
  if (p.taps) {  // one launch, two planes (the last layer: the skip sum only)
    if (!last) CHECK(p.tap(tap_name("blk%d.h%d", blk, j), dv.h, H));
    CHECK(p.tap(tap_name("blk%d.skip%d", blk, j), dv.skip, H, !last));
  }
  return 0;
}

// Flow block `blk` in reverse (CouplingBlock, attentions.py:119-142; WN.forward, layers.py:138-162).  Three forms of the same
// arithmetic, fastest first:
//   * the WaveNet: the fp16 mode's one launch for every layer but the last tail (wn16), else per layer the 16-row gate tile or
//     the generic tile, and res_skip on the 16-row tile or the generic one;
//   * the tail: last res_skip + end + coupling + InvConvNear / ActNorm + the NEXT block's start conv in one launch (tail_done),
//     else res_skip, then the coupling conv with the mix in its epilogue, else the mix as a launch of its own.
// *start_done: in, the previous block's tail already ran this block's start conv; out, this block's tail ran the next one's.
static int glow_flow_block(const GlowPass& p, const GlowDecView& dv, const float* spk_cond, bool glow_f16, int blk, bool* start_done) {
  const mi355tts_glow_hparams& h = p.gm->hp;
  const GlowBlock& Bk = p.gm->blocks[blk];
  const int H = h.hidden_channels, C = h.mel_channels * h.n_sqz, half = C / 2, F2 = p.ld, n = h.n_block_layers;
  const long long bsZ = (long long)C * F2, bsD = (long long)H * F2;
  float* const hcur = dv.h;  // the WaveNet's hidden state
  if (!*start_done) {
    CHECK(p.conv(Bk.start, p.args(dv.z, bsZ, hcur, bsD)));  // h = start(x0)
    if (p.taps) CHECK(p.tap(tap_name("blk%d.h", blk), hcur, H));
  }
  *start_done = false;
  int dil = 1;
  // the fp16 mode: layers 0 .. n - 1 up to the last gated tile in ONE launch (wn_f16.h); the loop then runs the last layer's tail
  const bool wn16 = glow_f16 && run_wn_f16(p, dv, Bk) == 0;
  if (wn16 && p.taps) {  // the launch keeps the layers between in LDS: the last layer's gated activations and the skip sum before it
    CHECK(p.tap(tap_name("blk%d.acts%d", blk, n - 1), dv.acts, H));
    if (n > 1) CHECK(p.tap(tap_name("blk%d.skip%d", blk, n - 2), dv.skip, H, true));
  }
  for (int j = wn16 ? n - 1 : 0; j < n; ++j) {
    const bool last = j == n - 1;
    if (!wn16) CHECK(glow_wn_gate(p, dv, spk_cond, blk, j, dil));
    if (last) {
      const GlowBlock* next = blk > 0 ? &p.gm->blocks[blk - 1] : nullptr;
      *start_done = run_glow_tail(p, dv, Bk, next) == 0;
      if (*start_done && p.taps) {
        CHECK(p.tap(tap_name("blk%d.z", blk), dv.z, C));
        if (next) CHECK(p.tap(tap_name("blk%d.h", blk - 1), dv.h, H, true));
      }
      if (*start_done) return 0;
    }
    CHECK(glow_wn_res_skip(p, dv, Bk, j, blk));
    dil *= h.dilation_rate;
  }
  // m, logs = end(wn_out);  z1 = (x1 - m) * exp(-logs)
  float* z1 = dv.z + (size_t)half * F2;
  ConvArgs a = p.args(dv.skip, bsD, z1, bsZ);
  a.res = z1;
  a.half = half;
  const bool fuse_mix = h.n_split == 4 && (half % 2) == 0;
  if (fuse_mix) {  // InvConvNear + ActNorm ride in the coupling conv's epilogue
    a.mix_x0 = dv.z; a.mix_w = p.A + Bk.winv; a.mix_bias = p.A + Bk.an_bias; a.mix_scale = p.A + Bk.an_scale;
  }
  CHECK(p.conv(Bk.end, a, EPI_COUPLING));
  if (fuse_mix) return p.taps ? p.tap(tap_name("blk%d.z", blk), dv.z, C) : 0;
  if (p.taps) CHECK(p.tap(tap_name("blk%d.zc", blk), dv.z, C));
  {
    ProfScope ps = p.small();
    hipLaunchKernelGGL(invconv_actnorm_kernel, dim3((p.n_max + 255) / 256, std::min(C / h.n_split, 16), p.B), dim3(256), 0, p.s, dv.z, bsZ, F2,
                       p.d_len, 1, C, h.n_split, p.A + Bk.winv, p.A + Bk.an_bias, p.A + Bk.an_scale);
  }
  return p.taps ? p.tap(tap_name("blk%d.z", blk), dv.z, C) : 0;
}

static int glow_decoder(GlowRun& r) {
  const GlowCall& call = r.call;
  const mi355tts_glow_hparams& h = r.gm->hp;
  Worker* w = r.w;
  hipStream_t s = w->stream;
  mi355tts_mel* mel = r.mel;
  const int B = call.B, M = h.mel_channels, nsq = h.n_sqz, P = r.el.P;
  const int Fmax = mel->max_frames, Fld = mel->ld, F2max = Fmax / nsq, F2 = (F2max + 3) & ~3;
  const long long bsZ = (long long)M * nsq * F2;
  const bool host_noise = call.noise && !(call.flags & MI355TTS_IN_DEVICE);
  GlowDecView dv;
  CHECK(glow_dec_workspace(r, glow_dec_layout(h, r.el.total, B, Fmax, host_noise ? (size_t)B * M * call.noise_ld : 0), &dv));
  const GlowEncView& v = r.ev;
  const float* d_noise = call.noise;
  if (host_noise) {
    HIPCHECK(hipMemcpyAsync(dv.nz, call.noise, sizeof(float) * (size_t)B * M * call.noise_ld, hipMemcpyHostToDevice, s));
    d_noise = dv.nz;
  }
  {
    ProfScope ps(r.ctx, w, KC_SMALL, 0);
    hipLaunchKernelGGL(expand_noise_squeeze_kernel, dim3((Fmax + 255) / 256, 8, B), dim3(256), 0, s, v.xm, (long long)M * P, P, v.len,
                       v.cum, P, mel->frames_dev, d_noise, (long long)M * call.noise_ld, call.noise_ld, call.noise_scale, call.seed,
                       call.row_seeds ? v.seeds : nullptr, M, nsq, dv.z, bsZ, F2);
  }
  // the decoder's time axis: row b is frames[b] / n_sqz columns long (frames are multiples of n_sqz), computed on the host side
  // of the sync.  The array reuses the id lengths' slot: they are no longer needed after expansion.
  int* d_f2 = v.len;
  for (int b = 0; b < B; ++b) w->pinned[b] = mel->frames[b] / nsq;
  HIPCHECK(hipMemcpyAsync(d_f2, w->pinned, sizeof(int) * B, hipMemcpyHostToDevice, s));
  // (w->pinned holds the rows' decoder lengths until the end of the pass: nothing below stages through it)
  const GlowPass p = r.pass(F2max, F2, d_f2, B == 1 ? mel->frames[0] / nsq : -1, KC_GLOW_DEC_CONV, w->pinned);
  if (p.taps) CHECK(p.tap("z0", dv.z, M * nsq));
  // the `half` switch as this call saw it: the decoder's WaveNets in fp16 (wn_f16.h)
  const bool glow_f16 = r.gm->f16_ok && r.gm->precision.load() == MI355TTS_PRECISION_F16;
  bool start_done = false;
  for (int blk = h.n_blocks_dec - 1; blk >= 0; --blk)
    CHECK(glow_flow_block(p, dv, r.gm->gin() ? v.cond : nullptr, glow_f16, blk, &start_done));
  {
    ProfScope ps(r.ctx, w, KC_SMALL, 0);
    hipLaunchKernelGGL(mel_finalize_kernel, dim3((Fld + 255) / 256, std::min(M, 16), B), dim3(256), 0, s, dv.z, bsZ, F2, mel->frames_dev, M,
                       nsq, mel->raw, mel->voc, (long long)M * Fld, Fld, to_mt(call.audio), call.audio ? 1 : 0);
  }
  return p.taps ? p.taps->add(s, "mel", mel->raw, false, B, M, Fld, mel->frames.data(), false) : 0;
}

// The forward pass on frame `f`, which holds the mel (f.mel) from the moment it exists.  With `final_sync` false the mel's last
// kernels are still queued on f.s when this returns (the fused synthesize path launches the vocoder behind them on the same
// stream).
static int glow_run(CallFrame& f, const GlowModel* gm, const GlowCall& call, int Pmax, bool final_sync) {
  Worker* w = f.w;
  const int glow_tiles = call.solo_tiles ? (1 << 30) : w->opt.env.glow_tiles > 0 ? w->opt.env.glow_tiles : 1024;
  GlowRun r{f.ctx, w, gm, call, Pmax, glow_tiles, glow_enc_layout(gm->hp, call.B, call.ids_ld, Pmax), {}, nullptr};
  if (call.taps && (call.row_ids || call.solo_tiles)) return fail(MI355TTS_ERR_INVALID, "the rows of a coalesced pass cannot be tapped: a call of its own");
  TapNames kn_out(w, call.taps);
  CHECK(glow_encoder(r));
  CHECK(glow_durations(r, f));
  if (r.mel->max_frames == 0) f.done = true;  // nothing to decode, and glow_durations has waited for all there was
  else CHECK(glow_decoder(r));
  return final_sync && !f.done ? f.finish() : 0;
}

// the arguments the entry points share, in their order (the rest of a GlowCall is filled by the entry that has it)
static GlowCall glow_call(const int64_t* ids, const int32_t* id_lens, int B, int ids_ld, float noise_scale, float length_scale,
                          const float* noise, int noise_ld, uint64_t seed, const mi355tts_audio_settings* audio, uint32_t flags) {
  GlowCall c;
  c.ids = ids; c.id_lens = id_lens; c.B = B; c.ids_ld = ids_ld;
  c.noise_scale = noise_scale; c.length_scale = length_scale;
  c.noise = noise; c.noise_ld = noise_ld; c.seed = seed;
  c.audio = audio; c.flags = flags;
  return c;
}

static int glow_infer_impl(mi355tts_ctx* ctx, int glow, const GlowCall& c, mi355tts_mel** out) {
  if (!ctx || !out) return fail(MI355TTS_ERR_INVALID, "null argument");
  std::shared_ptr<GlowModel> gpin;
  CHECK(find_model(ctx, glow, &gpin));
  const GlowModel* gm = gpin.get();
  int Pmax = 0;
  CHECK(glow_precheck(gm, c, &Pmax));
  CallFrame f(ctx);
  CHECK(f.open());
  CHECK(glow_run(f, gm, c, Pmax, true));
  *out = f.take_mel();
  return 0;
}

extern "C" int mi355tts_glow_infer(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                                   float noise_scale, float length_scale, const float* noise, int noise_ld, uint64_t seed,
                                   const mi355tts_audio_settings* audio, uint32_t flags, mi355tts_mel** out) {
  return glow_infer_impl(ctx, glow, glow_call(ids, id_lens, B, ids_ld, noise_scale, length_scale, noise, noise_ld, seed, audio, flags), out);
}
extern "C" int mi355tts_glow_infer_speakers(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                                            float noise_scale, float length_scale, const float* noise, int noise_ld, uint64_t seed,
                                            const uint64_t* row_seeds, const int32_t* speaker_ids, const mi355tts_audio_settings* audio,
                                            uint32_t flags, mi355tts_mel** out) {
  if (!speaker_ids) return fail(MI355TTS_ERR_INVALID, "speaker_ids null");
  GlowCall c = glow_call(ids, id_lens, B, ids_ld, noise_scale, length_scale, noise, noise_ld, seed, audio, flags);
  c.row_seeds = row_seeds;
  c.speaker_ids = speaker_ids;
  return glow_infer_impl(ctx, glow, c, out);
}
extern "C" int mi355tts_glow_infer_rows(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                                        float noise_scale, float length_scale, const uint64_t* row_seeds,
                                        const mi355tts_audio_settings* audio, uint32_t flags, mi355tts_mel** out) {
  if (!row_seeds) return fail(MI355TTS_ERR_INVALID, "row_seeds null");
  GlowCall c = glow_call(ids, id_lens, B, ids_ld, noise_scale, length_scale, nullptr, 0, 0, audio, flags);
  c.row_seeds = row_seeds;
  return glow_infer_impl(ctx, glow, c, out);
}
extern "C" int mi355tts_glow_infer_prosody(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                                           float noise_scale, float length_scale, const float* noise, int noise_ld, uint64_t seed,
                                           const uint64_t* row_seeds, const int32_t* speaker_ids, const mi355tts_audio_settings* audio,
                                           uint32_t flags, const mi355tts_prosody* prosody, mi355tts_mel** out) {
  GlowCall c = glow_call(ids, id_lens, B, ids_ld, noise_scale, length_scale, noise, noise_ld, seed, audio, flags);
  c.row_seeds = row_seeds;
  c.speaker_ids = speaker_ids;
  c.set_prosody(prosody, true);  // the two-call form: the mel always keeps the durations
  return glow_infer_impl(ctx, glow, c, out);
}

// ------------------------------------------------------------------ the test seam's entry point (the store and the read-out: host_taps.h)
extern "C" int mi355tts_glow_infer_taps(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                                        float noise_scale, float length_scale, const float* noise, int noise_ld, uint64_t seed,
                                        const uint64_t* row_seeds, const int32_t* speaker_ids, const mi355tts_audio_settings* audio,
                                        uint32_t flags, const mi355tts_prosody* prosody, mi355tts_mel** out, char* json, int cap) {
  if (!json) return fail(MI355TTS_ERR_INVALID, "null argument");
  auto taps = std::make_shared<VocTaps>();
  GlowCall c = glow_call(ids, id_lens, B, ids_ld, noise_scale, length_scale, noise, noise_ld, seed, audio, flags);
  c.row_seeds = row_seeds;
  c.speaker_ids = speaker_ids;
  c.set_prosody(prosody, true);
  c.taps = taps.get();
  CHECK(glow_infer_impl(ctx, glow, c, out));  // (ends with the stream synchronised: the copies are complete)
  const int rc = finish_taps(ctx, taps, json, cap);
  if (rc) {
    mel_destroy(*out);
    *out = nullptr;
  }
  return rc;
}
