// mi355tts host runtime — forced alignment: mi355tts_glow_align (encoder as in a synthesis call, the decoder's flows FORWARDS,
// mel -> z: glow_tts/models.py:191-209 with reverse=False, the scores, the best monotonic path: glow_tts/utils.py:59-96) and
// the single operator mi355tts_op_maximum_path.  Kernels: align.h, glow_fwd_kernel (coltile.h).
// (one translation unit: included once by mi355tts.hip, after glow_forward.h; the call frame and the model table: host_call.h)
#pragma once

// ids per lane of the path kernel's one wave: the smallest of 1, 2, 4, .. 32 that covers P
static int path_chunk(int Pmax) {
  int ch = 1;
  while (64 * ch < Pmax) ch *= 2;
  return ch;
}

// The alignment's own buffers, appended to the encoder's and the decoder's regions: ONE definition for the call and
// mi355tts_reserve.  `ldp` is the id stride of the time-major score matrix (whole waves of the path kernel).
struct AlignLayout {
  size_t o_frames, o_f2, o_plen, o_mz, o_ml, o_lp, o_bits, o_dur, o_score, total;
  int CH, ldp, dur_ld;
  long long bits_bs;  // words of direction bits per row (0: every row's bits fit the path kernel's LDS)
};
static AlignLayout align_layout(size_t base, int B, int Pmax, int Fmax, size_t mz_floats, size_t ml_floats) {
  AlignLayout L;
  L.CH = path_chunk(Pmax);
  L.ldp = 64 * L.CH;
  L.dur_ld = (Pmax + 3) & ~3;
  const long long words = (long long)Fmax * 2 * L.CH;
  L.bits_bs = words > PATH_LDS_WORDS ? words : 0;
  Carver cv;
  cv.pos = base;
  L.o_frames = cv.take(sizeof(int) * B);
  L.o_f2 = cv.take(sizeof(int) * B);
  L.o_plen = cv.take(sizeof(int) * B);
  L.o_mz = cv.take(sizeof(float) * mz_floats);
  L.o_ml = cv.take(sizeof(float) * ml_floats);
  L.o_lp = cv.take(sizeof(float) * (size_t)B * Fmax * L.ldp);
  L.o_bits = cv.take(sizeof(unsigned) * (size_t)B * L.bits_bs);
  L.o_dur = cv.take(sizeof(int) * (size_t)B * L.dur_ld);
  L.o_score = cv.take(sizeof(float) * B);
  L.total = cv.pos;
  return L;
}
// what mi355tts_glow_align carves for a model: the encoder's region, the decoder's, then the alignment's
static AlignLayout glow_align_layout(const mi355tts_glow_hparams& h, const GlowEncLayout& el, int B, int Pmax, int Fmax, int mel_ld,
                                     GlowDecLayout* dl_out) {
  const GlowDecLayout dl = glow_dec_layout(h, el.total, B, Fmax, 0);
  if (dl_out) *dl_out = dl;
  const size_t F2 = (size_t)((Fmax / h.n_sqz + 3) & ~3);
  return align_layout(dl.total, B, Pmax, Fmax, (size_t)B * h.mel_channels * mel_ld, (size_t)B * h.mel_channels * h.n_sqz * F2);
}

static void launch_path(mi355tts_ctx* ctx, Worker* w, const AlignLayout& al, int B, const float* logp, long long lp_bs, const int* d_plen,
                        const int* d_frames, unsigned* bits, int* dur, float* score) {
  ProfScope ps(ctx, w, KC_SMALL, 0);
  ps.kernel(KN_ALIGN_PATH);
  switch_const<1, 2, 4, 8, 16, 32>(al.CH, [&](auto ch) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(align_path_kernel<decltype(ch)::value>), dim3(B), dim3(64), 0, w->stream, logp, lp_bs, al.ldp, d_plen,
                       d_frames, bits, al.bits_bs, dur, al.dur_ld, score);
  });
}

// durations and scores: device -> pinned staging (behind whatever the caller queued there first) -> the caller's arrays
static int align_results(CallFrame& f, const AlignLayout& al, const int32_t* id_lens, int B, const int* d_dur, const float* d_score,
                         size_t staged, int32_t* durations_out, int dur_ld, float* score_out) {
  const size_t dur_b = sizeof(int) * (size_t)B * al.dur_ld;
  char* pd = f.w->pinned_out + staged;
  char* psc = pd + dur_b;
  HIPCHECK(hipMemcpyAsync(pd, d_dur, dur_b, hipMemcpyDeviceToHost, f.s));
  HIPCHECK(hipMemcpyAsync(psc, d_score, sizeof(float) * B, hipMemcpyDeviceToHost, f.s));
  CHECK(f.finish());
  for (int b = 0; b < B; ++b) {
    int32_t* dst = durations_out + (size_t)b * dur_ld;
    std::memset(dst, 0, sizeof(int32_t) * (size_t)dur_ld);
    std::memcpy(dst, (const int*)pd + (size_t)b * al.dur_ld, sizeof(int32_t) * (size_t)id_lens[b]);
  }
  if (score_out) std::memcpy(score_out, psc, sizeof(float) * B);
  return 0;
}

// the path's own limits, shared by both entries; *Fmax_out: the longest row
static int path_precheck(const int32_t* id_lens, const int32_t* frames, int B, int dur_ld, int* Pmax_out, int* Fmax_out) {
  int Pmax = 0, Fmax = 0;
  for (int b = 0; b < B; ++b) {
    if (id_lens[b] > PATH_MAX_P)
      return fail(MI355TTS_ERR_INVALID, "id_lens[%d]=%d: the path kernel holds at most %d ids per row (64 lanes x 32)", b, id_lens[b], PATH_MAX_P);
    if (frames[b] < id_lens[b])
      return fail(MI355TTS_ERR_INVALID, "row %d has %d frames for %d ids: a monotonic path gives every id at least one frame", b, frames[b],
                  id_lens[b]);
    if (dur_ld < id_lens[b]) return fail(MI355TTS_ERR_INVALID, "dur_ld %d < id_lens[%d]=%d", dur_ld, b, id_lens[b]);
    Pmax = std::max(Pmax, id_lens[b]);
    Fmax = std::max(Fmax, frames[b]);
  }
  *Pmax_out = Pmax;
  *Fmax_out = Fmax;
  return 0;
}

// ---- the forward flow
// the seam between block `prev` (nullptr: in front of block 0) and block `next` (nullptr: behind the last block) in one
// launch (glow_fwd_kernel); 1 = not a shape the kernel takes
static int run_glow_fwd(const GlowPass& p, const GlowDecView& dv, const GlowBlock* prev, const GlowBlock* next) {
  const mi355tts_glow_hparams& h = p.gm->hp;
  const int H = h.hidden_channels, half = h.mel_channels * h.n_sqz / 2, F2 = p.ld;
  if (!glow_fuse_on(p.w) || (prev && (!prev->t_rs.ok || !prev->t_end.ok)) || (next && !next->t_st.ok) || (!prev && !next) || h.n_split != 4 ||
      (half % 2) || 2 * half > COL_MAXROWS || H > COL_MAXROWS || F2 % 4 || p.n_max <= 0)
    return 1;
  const float* A = p.A;
  GlowFwdArgs a;
  std::memset(&a, 0, sizeof(a));
  a.acts = dv.acts; a.skip = h.n_block_layers > 1 ? dv.skip : nullptr; a.hnext = next ? dv.h : nullptr; a.h_bs = (long long)H * F2; a.h_ld = F2;
  a.z = dv.z; a.z_bs = (long long)h.mel_channels * h.n_sqz * F2; a.z_ld = F2;
  p.rows().into(a);
  a.len_mul = 1;
  if (prev) {
    a.w_rs = A + prev->t_rs.w_off; a.b_rs = A + prev->t_rs.b_off;
    a.w_end = A + prev->t_end.w_off; a.b_end = A + prev->t_end.b_off;
  }
  const GlowBlock& nb = next ? *next : *prev;  // the last block has no successor: its own constants stand in (loaded, never used)
  a.w_st = A + nb.t_st.w_off; a.b_st = A + nb.t_st.b_off;
  a.mix_w = A + nb.wfwd; a.mix_bias = A + nb.an_bias; a.mix_scale = A + nb.an_escale;
  a.H = H; a.half = half;
  const double mac = (prev ? (double)H * H + 2.0 * half * H : 0.0) + (next ? (double)H * half : 0.0);
  ProfScope ps(p.ctx, p.w, p.cls, 2.0 * mac * (double)p.n_max * p.B);
  ps.kernel(KN_GLOW_FWD);
  const dim3 grid((p.n_max + COL_T - 1) / COL_T, p.B);
  if (prev) hipLaunchKernelGGL(glow_fwd_kernel<true>, grid, dim3(512), 0, p.s, a);
  else hipLaunchKernelGGL(glow_fwd_kernel<false>, grid, dim3(512), 0, p.s, a);
  return 0;
}

// Flow block `blk` forwards (ActNorm, InvConvNear, CouplingBlock with reverse=False).  *start_done: in, the previous launch
// already ran this block's ActNorm + InvConvNear + start; out, this block's last launch ran the next block's.  The un-fused
// form: the mix as a launch of its own, start, the WaveNet, res_skip, end into `ml`, the coupling as a launch of its own.
static int glow_flow_block_fwd(const GlowPass& p, const GlowDecView& dv, float* ml, const float* spk_cond, int blk, bool* start_done) {
  const mi355tts_glow_hparams& h = p.gm->hp;
  const GlowBlock& Bk = p.gm->blocks[blk];
  const int H = h.hidden_channels, C = h.mel_channels * h.n_sqz, half = C / 2, F2 = p.ld, n = h.n_block_layers;
  const long long bsZ = (long long)C * F2, bsD = (long long)H * F2;
  if (!*start_done) {
    {
      ProfScope ps = p.small();
      hipLaunchKernelGGL(actnorm_invconv_fwd_kernel, dim3((p.n_max + 255) / 256, std::min(C / h.n_split, 16), p.B), dim3(256), 0, p.s, dv.z, bsZ,
                         F2, p.d_len, C, h.n_split, p.A + Bk.wfwd, p.A + Bk.an_bias, p.A + Bk.an_escale);
    }
    CHECK(p.conv(Bk.start, p.args(dv.z, bsZ, dv.h, bsD)));  // h = start(x0)
  }
  *start_done = false;
  int dil = 1;
  for (int j = 0; j < n; ++j) {
    CHECK(glow_wn_gate(p, dv, spk_cond, blk, j, dil));
    if (j == n - 1) {
      const GlowBlock* next = blk + 1 < h.n_blocks_dec ? &p.gm->blocks[blk + 1] : nullptr;
      *start_done = run_glow_fwd(p, dv, &Bk, next) == 0;
      if (*start_done) {
        *start_done = next != nullptr;
        return 0;
      }
    }
    CHECK(glow_wn_res_skip(p, dv, Bk, j));
    dil *= h.dilation_rate;
  }
  // m, logs = end(wn_out);  z1 = m + exp(logs) * x1
  CHECK(p.conv(Bk.end_lin, p.args(dv.skip, bsD, ml, bsZ)));
  ProfScope ps = p.small();
  hipLaunchKernelGGL(coupling_fwd_kernel, dim3((p.n_max + 255) / 256, std::min(half, 16), p.B), dim3(256), 0, p.s, dv.z, ml, bsZ, F2, p.d_len,
                     half);
  return 0;
}

extern "C" int mi355tts_glow_align(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                                   const float* mel, const int32_t* frames, int mel_ld, const int32_t* speaker_ids, uint32_t flags,
                                   int32_t* durations_out, int dur_ld, float* score_out, float* z_out) {
  if (!ctx || !mel || !frames || !durations_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  std::shared_ptr<GlowModel> gpin;
  CHECK(find_model(ctx, glow, &gpin));
  const GlowModel* gm = gpin.get();
  const mi355tts_glow_hparams& h = gm->hp;
  GlowCall call = glow_call(ids, id_lens, B, ids_ld, 0.f, 1.f, nullptr, 0, 0, nullptr, 0);
  call.speaker_ids = speaker_ids;
  int Pmax = 0, Fmax = 0;
  CHECK(glow_precheck(gm, call, &Pmax));
  if (mel_ld < 1) return fail(MI355TTS_ERR_INVALID, "mel_ld %d < 1", mel_ld);
  if (h.mel_channels > SC_MAXM) return fail(MI355TTS_ERR_INVALID, "mel_channels %d > %d: not covered by the score kernel", h.mel_channels, SC_MAXM);
  const int M = h.mel_channels, nsq = h.n_sqz;
  std::vector<int32_t> F(B);
  for (int b = 0; b < B; ++b) {
    if (frames[b] < 0 || frames[b] > mel_ld) return fail(MI355TTS_ERR_INVALID, "frames[%d]=%d outside [0, mel_ld=%d]", b, frames[b], mel_ld);
    F[b] = frames[b] / nsq * nsq;  // FlowGenerator.preprocess, models.py:356-363: later frames are ignored
  }
  CHECK(path_precheck(id_lens, F.data(), B, dur_ld, &Pmax, &Fmax));
  const bool in_dev = (flags & MI355TTS_IN_DEVICE) != 0, out_dev = (flags & MI355TTS_OUT_DEVICE) != 0;
  CallFrame f(ctx);
  CHECK(f.open());
  Worker* w = f.w;
  hipStream_t s = f.s;
  const int glow_tiles = w->opt.env.glow_tiles > 0 ? w->opt.env.glow_tiles : 1024;
  GlowRun r{ctx, w, gm, call, Pmax, glow_tiles, glow_enc_layout(h, B, ids_ld, Pmax), {}, nullptr};
  // every size is known up front (unlike a synthesis call's frame count): the arena is sized once, before the encoder binds it
  GlowDecLayout dl;
  const AlignLayout al = glow_align_layout(h, r.el, B, Pmax, Fmax, mel_ld, &dl);
  const size_t z_b = z_out && !out_dev ? sizeof(float) * (size_t)B * M * mel_ld : 0;
  CHECK(f.reserve(al.total, z_b + sizeof(int) * (size_t)B * al.dur_ld + sizeof(float) * B));
  CHECK(f.pinned_ints((size_t)3 * B));
  CHECK(glow_encoder(r));
  const GlowEncView& v = r.ev;
  char* base = w->arena;
  const GlowDecView dv = glow_dec_view(dl, base);
  int* d_frames = (int*)(base + al.o_frames);
  int* d_f2 = (int*)(base + al.o_f2);
  float* mz = (float*)(base + al.o_mz);
  float* ml = (float*)(base + al.o_ml);
  float* logp = (float*)(base + al.o_lp);
  int* d_dur = (int*)(base + al.o_dur);
  float* d_score = (float*)(base + al.o_score);
  long long sum = 0;
  for (int b = 0; b < B; ++b) {
    w->pinned[b] = F[b];
    w->pinned[B + b] = F[b] / nsq;
    sum += F[b];
  }
  w->flop_scale = (double)sum / ((double)B * Fmax);
  HIPCHECK(hipMemcpyAsync(d_frames, w->pinned, sizeof(int) * B, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(d_f2, w->pinned + B, sizeof(int) * B, hipMemcpyHostToDevice, s));
  const float* d_mel = mel;
  if (!in_dev) {
    HIPCHECK(hipMemcpyAsync(mz, mel, sizeof(float) * (size_t)B * M * mel_ld, hipMemcpyHostToDevice, s));
    d_mel = mz;
  }
  // ---- the decoder forwards: squeeze, the flow blocks in ascending order, unsqueeze.  Always f32: an alignment does not depend
  // on the `half` switch.
  const int F2max = Fmax / nsq, F2 = (F2max + 3) & ~3;
  const long long bsZ = (long long)M * nsq * F2, bsM = (long long)M * mel_ld;
  {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    hipLaunchKernelGGL(mel_squeeze_kernel, dim3((F2 + 255) / 256, std::min(M, 16), B), dim3(256), 0, s, d_mel, bsM, mel_ld, d_frames, M, nsq, dv.z,
                       bsZ, F2);
  }
  const GlowPass p = r.pass(F2max, F2, d_f2, B == 1 ? F[0] / nsq : -1, KC_GLOW_DEC_CONV);
  bool start_done = h.n_blocks_dec > 0 && run_glow_fwd(p, dv, nullptr, &gm->blocks[0]) == 0;
  for (int blk = 0; blk < h.n_blocks_dec; ++blk) CHECK(glow_flow_block_fwd(p, dv, ml, gm->gin() ? v.cond : nullptr, blk, &start_done));
  float* d_z = z_out && out_dev ? z_out : mz;  // (the staged mel has been consumed by the squeeze)
  {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    hipLaunchKernelGGL(z_unsqueeze_kernel, dim3((mel_ld + 255) / 256, std::min(M, 16), B), dim3(256), 0, s, dv.z, bsZ, F2, d_frames, M, nsq, d_z,
                       bsM, mel_ld);
  }
  // ---- scores, path
  const long long lp_bs = (long long)Fmax * al.ldp;
  {
    ProfScope ps(ctx, w, KC_SMALL, 2.0 * M * (double)Pmax * Fmax * B);
    ps.kernel(KN_ALIGN_SCORE);
    const float c0 = (float)(-0.5 * M * std::log(2.0 * 3.14159265358979323846));
    hipLaunchKernelGGL(align_score_kernel, dim3(al.ldp / 64, (Fmax + SC_TJ - 1) / SC_TJ, B), dim3(256), 0, s, v.xm, (long long)M * r.el.P, r.el.P,
                       v.len, d_z, bsM, mel_ld, d_frames, M, c0, logp, lp_bs, al.ldp);
  }
  launch_path(ctx, w, al, B, logp, lp_bs, v.len, d_frames, (unsigned*)(base + al.o_bits), d_dur, d_score);
  if (z_b) HIPCHECK(hipMemcpyAsync(w->pinned_out, d_z, z_b, hipMemcpyDeviceToHost, s));
  CHECK(align_results(f, al, id_lens, B, d_dur, d_score, z_b, durations_out, dur_ld, score_out));
  if (z_b) std::memcpy(z_out, w->pinned_out, z_b);
  return 0;
}

extern "C" int mi355tts_op_maximum_path(mi355tts_ctx* ctx, const float* value, int B, int P_ld, int F_ld, const int32_t* id_lens,
                                        const int32_t* frames, int32_t* durations_out, int dur_ld, float* score_out) {
  if (!ctx || !value || !id_lens || !frames || !durations_out) return fail(MI355TTS_ERR_INVALID, "null argument");
  if (B <= 0 || P_ld <= 0 || F_ld <= 0) return fail(MI355TTS_ERR_INVALID, "empty batch");
  for (int b = 0; b < B; ++b)
    if (id_lens[b] < 1 || id_lens[b] > P_ld || frames[b] < 1 || frames[b] > F_ld)
      return fail(MI355TTS_ERR_INVALID, "row %d: %d x %d outside [1, %d] x [1, %d]", b, id_lens[b], frames[b], P_ld, F_ld);
  int Pmax = 0, Fmax = 0;
  CHECK(path_precheck(id_lens, frames, B, dur_ld, &Pmax, &Fmax));
  CallFrame f(ctx);
  CHECK(f.open());
  Worker* w = f.w;
  hipStream_t s = f.s;
  const size_t nval = (size_t)B * P_ld * F_ld;
  const AlignLayout al = align_layout(0, B, Pmax, Fmax, nval, 0);
  CHECK(f.reserve(al.total, sizeof(int) * (size_t)B * al.dur_ld + sizeof(float) * B));
  CHECK(f.pinned_ints((size_t)2 * B));
  char* base = w->arena;
  int* d_frames = (int*)(base + al.o_frames);
  int* d_plen = (int*)(base + al.o_plen);
  float* d_val = (float*)(base + al.o_mz);
  float* logp = (float*)(base + al.o_lp);
  for (int b = 0; b < B; ++b) {
    w->pinned[b] = frames[b];
    w->pinned[B + b] = id_lens[b];
  }
  HIPCHECK(hipMemcpyAsync(d_frames, w->pinned, sizeof(int) * B, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(d_plen, w->pinned + B, sizeof(int) * B, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(d_val, value, sizeof(float) * nval, hipMemcpyHostToDevice, s));
  const long long lp_bs = (long long)Fmax * al.ldp;
  {
    ProfScope ps(ctx, w, KC_SMALL, 0);
    hipLaunchKernelGGL(path_transpose_kernel, dim3((al.ldp + 255) / 256, Fmax, B), dim3(256), 0, s, d_val, P_ld, F_ld, d_plen, d_frames, logp, lp_bs,
                       al.ldp, Fmax);
  }
  launch_path(ctx, w, al, B, logp, lp_bs, d_plen, d_frames, (unsigned*)(base + al.o_bits), (int*)(base + al.o_dur), (float*)(base + al.o_score));
  return align_results(f, al, id_lens, B, (int*)(base + al.o_dur), (float*)(base + al.o_score), 0, durations_out, dur_ld, score_out);
}
