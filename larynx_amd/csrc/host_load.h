// mi355tts host runtime — model loading: a weight blob in manifest order becomes a model.  BlobReader walks the blob against
// the manifest, build_glow_model / build_hifi_model pack every tensor into a ModelPacker's host arenas (stage by stage, in the
// order of the manifest), ModelPacker::upload moves the arenas to the device and binds every conv the model's each_conv
// visits.  The C ABI's loaders (mi355tts.hip) are open_blob -> build -> upload -> register_model (host_call.h).
// (one translation unit: included once by mi355tts.hip, after hifigan_f16.h for the fp16 packers)
#pragma once

// ------------------------------------------------------------------ reading the blob
struct WB {  // a conv's weight and bias, or a norm's gamma and beta
  const float* w = nullptr;
  const float* b = nullptr;
};
struct BlobReader {
  const float* p = nullptr;
  int64_t pos = 0;
  std::vector<std::pair<std::string, int64_t>> manifest;
  size_t idx = 0;
  // the next tensor of the manifest, which must be `name` with `numel` elements
  int take(const std::string& name, int64_t numel, const float** out) {
    if (idx >= manifest.size() || manifest[idx].first != name || manifest[idx].second != numel)
      return fail(MI355TTS_ERR_INVALID, "weight blob does not match manifest at '%s'", name.c_str());
    *out = p + pos;
    pos += numel;
    idx++;
    return 0;
  }
  int conv(const std::string& prefix, int Cout, int Cin, int K, WB* out) {
    CHECK(take(prefix + ".weight", (int64_t)Cout * Cin * K, &out->w));
    return take(prefix + ".bias", Cout, &out->b);
  }
  int norm(const std::string& prefix, int n, WB* out) {
    CHECK(take(prefix + ".gamma", n, &out->w));
    return take(prefix + ".beta", n, &out->b);
  }
};

// Open a caller's blob for reading against `manifest`.  The size is compared before anything is copied: a device-resident blob
// of the wrong size is rejected without a transfer.  `host` keeps the host copy of a device blob alive for the reader.
static int open_blob(mi355tts_ctx* ctx, const char* what, std::vector<std::pair<std::string, int64_t>> manifest, const float* blob,
                     int64_t numel, int on_device, std::vector<float>& host, BlobReader* r) {
  int64_t total = 0;
  for (auto& kv : manifest) total += kv.second;
  if (total != numel) return fail(MI355TTS_ERR_INVALID, "%s blob has %lld floats, manifest needs %lld", what, (long long)numel, (long long)total);
  r->manifest = std::move(manifest);
  r->p = blob;
  if (!on_device) return 0;
  HIPCHECK(hipSetDevice(ctx->device));
  host.resize((size_t)numel);
  HIPCHECK(hipMemcpy(host.data(), blob, (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
  r->p = host.data();
  return 0;
}

// ------------------------------------------------------------------ host arenas -> device
template <class T>
static int upload_arena(const std::vector<T>& host, T** dev, const char* what) {
  hipError_t e = hipMalloc(dev, host.size() * sizeof(T) + 256);  // (slack: the kernels' prefetch may read past the last fragment)
  if (e != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc %s: %s", what, hipGetErrorString(e));
  HIPCHECK(hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
template <class Model>
int ModelPacker::upload(mi355tts_ctx* ctx, Model& model) {
  HIPCHECK(hipSetDevice(ctx->device));
  CHECK(upload_arena(f32.host, &model.arena, "model arena"));
  if (!bf16.empty()) CHECK(upload_arena(bf16, &model.arena16, "bf16 weight arena"));
  if (!f16.empty()) CHECK(upload_arena(f16, &model.arenaH, "fp16 weight arena"));
  const ArenaPtrs arenas = model.ptrs();
  model.each_conv([&](auto& c) { bind(c, arenas); });
  return 0;
}

// The single operators and the dispatcher self-check pack a conv or three into an ArenaBuilder and run them out of the worker's
// workspace: take the space (before the site's reserve), then copy on the worker's stream and bind (after it).
struct WorkerWeights {
  const ArenaBuilder& ab;
  size_t off;
  WorkerWeights(const ArenaBuilder& ab_, Carver& cv) : ab(ab_), off(cv.take(ab_.host.size() * sizeof(float))) {}
  int copy_and_bind(Worker* w, DevConv* convs, int n) const {
    float* dw = (float*)(w->arena + off);
    HIPCHECK(hipMemcpyAsync(dw, ab.host.data(), ab.host.size() * sizeof(float), hipMemcpyHostToDevice, w->stream));
    for (int i = 0; i < n; ++i) bind(convs[i], ArenaPtrs{dw, nullptr, nullptr});
    return 0;
  }
};

// ------------------------------------------------------------------ GlowTTS
// a plain conv in its f32 tile packing and, where the shape has one, the lin16 packing
static DevConv add_plain_conv(ModelPacker& pk, const WB& t, int Cout, int Cin, int K) {
  DevConv d = add_conv(pk.f32, t.w, t.b, Cout, Cin, K, ROWS_PLAIN);
  add_lin16(pk.f32, d, t.w, t.b, Cout, Cin, K);
  return d;
}

static int build_glow_embeddings(const mi355tts_glow_hparams& h, BlobReader& r, ModelPacker& pk, GlowModel& gm) {
  const float* t;
  CHECK(r.take("encoder.emb.weight", (int64_t)h.num_symbols * h.hidden_channels, &t));
  gm.emb = pk.add(t, (size_t)h.num_symbols * h.hidden_channels);
  if (gm.gin()) {
    CHECK(r.take("emb_g.weight", (int64_t)h.n_speakers * gm.gin(), &t));
    gm.emb_g = pk.add(t, (size_t)h.n_speakers * gm.gin());
  }
  return 0;
}

static int build_glow_prenet(const mi355tts_glow_hparams& h, BlobReader& r, ModelPacker& pk, GlowModel& gm) {
  const int H = h.hidden_channels;
  WB c, n;
  for (int i = 0; i < h.prenet_layers; ++i) {
    CHECK(r.conv("encoder.pre.conv_layers." + std::to_string(i), H, H, h.prenet_kernel_size, &c));
    CHECK(r.norm("encoder.pre.norm_layers." + std::to_string(i), H, &n));
    gm.pre_conv.push_back(add_plain_conv(pk, c, H, H, h.prenet_kernel_size));
    gm.pre_g.push_back(pk.add(n.w, H));
    gm.pre_b.push_back(pk.add(n.b, H));
  }
  CHECK(r.conv("encoder.pre.proj", H, H, 1, &c));
  gm.pre_proj = add_plain_conv(pk, c, H, H, 1);
  return 0;
}

static int build_glow_enc_layer(const mi355tts_glow_hparams& h, int l, BlobReader& r, ModelPacker& pk, GlowModel& gm) {
  const int H = h.hidden_channels, Fc = h.filter_channels, k = h.kernel_size;
  const int64_t nrel_dk = (int64_t)(2 * h.window_size + 1) * (H / h.n_heads);
  const std::string a = "encoder.encoder.attn_layers." + std::to_string(l), f = "encoder.encoder.ffn_layers." + std::to_string(l);
  GlowLayer L;
  const float *ek, *ev;
  WB q, kk, v, o, n1, c1, c2, n2;
  CHECK(r.take(a + ".emb_rel_k", nrel_dk, &ek));
  CHECK(r.take(a + ".emb_rel_v", nrel_dk, &ev));
  CHECK(r.conv(a + ".conv_q", H, H, 1, &q));
  CHECK(r.conv(a + ".conv_k", H, H, 1, &kk));
  CHECK(r.conv(a + ".conv_v", H, H, 1, &v));
  CHECK(r.conv(a + ".conv_o", H, H, 1, &o));
  // q, k, v share their input: one GEMM with 3H output rows (attentions.py:205-207)
  std::vector<float> wqkv, bqkv;
  for (const WB* t : {&q, &kk, &v}) {
    wqkv.insert(wqkv.end(), t->w, t->w + (size_t)H * H);
    bqkv.insert(bqkv.end(), t->b, t->b + H);
  }
  L.qkv = add_plain_conv(pk, WB{wqkv.data(), bqkv.data()}, 3 * H, H, 1);
  L.o = add_conv(pk.f32, o.w, o.b, H, H, 1, ROWS_PLAIN);
  L.o16 = add_col16(pk.f32, o.w, o.b, H, H);
  L.ek = pk.add(ek, (size_t)nrel_dk);
  L.ev = pk.add(ev, (size_t)nrel_dk);
  CHECK(r.norm("encoder.encoder.norm_layers_1." + std::to_string(l), H, &n1));
  L.g1 = pk.add(n1.w, H);
  L.b1 = pk.add(n1.b, H);
  CHECK(r.conv(f + ".conv_1", Fc, H, k, &c1));
  CHECK(r.conv(f + ".conv_2", H, Fc, k, &c2));
  L.ffn1 = add_conv(pk.f32, c1.w, c1.b, Fc, H, k, ROWS_PLAIN);
  L.ffn2 = add_conv(pk.f32, c2.w, c2.b, H, Fc, k, ROWS_PLAIN);
  add_lin16(pk.f32, L.ffn1, c1.w, c1.b, Fc, H, k);
  add_lin16(pk.f32, L.ffn2, c2.w, c2.b, H, Fc, k);
  CHECK(r.norm("encoder.encoder.norm_layers_2." + std::to_string(l), H, &n2));
  L.g2 = pk.add(n2.w, H);
  L.b2 = pk.add(n2.b, H);
  gm.layers.push_back(L);
  return 0;
}

// proj_m and the duration predictor (proj_w)
static int build_glow_projections(const mi355tts_glow_hparams& h, BlobReader& r, ModelPacker& pk, GlowModel& gm) {
  const int H = h.hidden_channels, Fd = h.filter_channels_dp, k = h.kernel_size, gin = gm.gin();
  WB m, c1, n1, c2, n2, pr;
  CHECK(r.conv("encoder.proj_m", h.mel_channels, H, 1, &m));
  gm.proj_m = add_plain_conv(pk, m, h.mel_channels, H, 1);
  CHECK(r.conv("encoder.proj_w.conv_1", Fd, H + gin, k, &c1));
  CHECK(r.norm("encoder.proj_w.norm_1", Fd, &n1));
  CHECK(r.conv("encoder.proj_w.conv_2", Fd, Fd, k, &c2));
  CHECK(r.norm("encoder.proj_w.norm_2", Fd, &n2));
  CHECK(r.conv("encoder.proj_w.proj", 1, Fd, 1, &pr));
  std::vector<float> w1x;  // multi-speaker: conv_1's weight is [Fd][H + gin][k]; the encoder half goes to the conv kernels
  if (gin) {
    std::vector<float> wg((size_t)Fd * gin * k);
    w1x.resize((size_t)Fd * H * k);
    for (int co = 0; co < Fd; ++co) {
      std::memcpy(&w1x[(size_t)co * H * k], c1.w + (size_t)co * (H + gin) * k, sizeof(float) * (size_t)H * k);
      std::memcpy(&wg[(size_t)co * gin * k], c1.w + ((size_t)co * (H + gin) + H) * k, sizeof(float) * (size_t)gin * k);
    }
    gm.dp_wg = pk.add(wg);
    c1.w = w1x.data();
  }
  gm.dp1 = add_conv(pk.f32, c1.w, c1.b, Fd, H, k, ROWS_PLAIN);
  gm.dp2 = add_conv(pk.f32, c2.w, c2.b, Fd, Fd, k, ROWS_PLAIN);
  add_lin16(pk.f32, gm.dp1, c1.w, c1.b, Fd, H, k);
  add_lin16(pk.f32, gm.dp2, c2.w, c2.b, Fd, Fd, k);
  gm.dpp = add_conv(pk.f32, pr.w, pr.b, 1, Fd, 1, ROWS_PLAIN);
  gm.dpp_w = pk.add(pr.w, Fd);
  gm.dpp_b = pk.add(pr.b, 1);
  gm.dg1 = pk.add(n1.w, Fd);
  gm.db1 = pk.add(n1.b, Fd);
  gm.dg2 = pk.add(n2.w, Fd);
  gm.db2 = pk.add(n2.b, Fd);
  return 0;
}

// out = in^-1 (n x n, row-major), Gauss-Jordan with partial pivoting in double; false when singular
static bool invert_small(const float* in, int n, std::vector<float>& out) {
  std::vector<double> a((size_t)n * 2 * n, 0.0);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) a[(size_t)i * 2 * n + j] = in[i * n + j];
    a[(size_t)i * 2 * n + n + i] = 1.0;
  }
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(a[(size_t)r * 2 * n + c]) > std::fabs(a[(size_t)piv * 2 * n + c])) piv = r;
    if (!(std::fabs(a[(size_t)piv * 2 * n + c]) > 0.0)) return false;
    for (int j = 0; j < 2 * n; ++j) std::swap(a[(size_t)c * 2 * n + j], a[(size_t)piv * 2 * n + j]);
    const double d = a[(size_t)c * 2 * n + c];
    for (int j = 0; j < 2 * n; ++j) a[(size_t)c * 2 * n + j] /= d;
    for (int r = 0; r < n; ++r) {
      const double f = a[(size_t)r * 2 * n + c];
      if (r == c || f == 0.0) continue;
      for (int j = 0; j < 2 * n; ++j) a[(size_t)r * 2 * n + j] -= f * a[(size_t)c * 2 * n + j];
    }
  }
  out.resize((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) out[(size_t)i * n + j] = (float)a[(size_t)i * 2 * n + n + j];
  return true;
}

// one flow block: ActNorm, InvConvNear, the coupling block's WaveNet.  cond_w / cond_b collect the blocks' cond_layer tensors.
static int build_glow_block(const mi355tts_glow_hparams& h, int b, BlobReader& r, ModelPacker& pk, GlowModel& gm,
                            std::vector<float>& cond_w, std::vector<float>& cond_b) {
  const int H = h.hidden_channels, C = h.mel_channels * h.n_sqz, half = C / 2, n = h.n_block_layers, Kd = h.kernel_size_dec;
  const std::string an = "decoder.flows." + std::to_string(3 * b), ic = "decoder.flows." + std::to_string(3 * b + 1);
  const std::string cp = "decoder.flows." + std::to_string(3 * b + 2);
  GlowBlock B;
  const float *logs, *abias, *winv;
  CHECK(r.take(an + ".logs", C, &logs));
  CHECK(r.take(an + ".bias", C, &abias));
  CHECK(r.take(ic + ".weight_inv", (int64_t)h.n_split * h.n_split, &winv));
  std::vector<float> scale(C);
  for (int c = 0; c < C; ++c) scale[c] = std::exp(-logs[c]);  // ActNorm reverse, layers.py:192-194
  B.an_bias = pk.add(abias, C);
  B.an_scale = pk.add(scale);
  B.winv = pk.add(winv, (size_t)h.n_split * h.n_split);
  // the flow forwards (forced alignment, align_forward.h): exp(+logs), and the forward n x n weight as the inverse of weight_inv
  // in double — the one form every loader can serve (an ONNX-exported voice carries only the inverse)
  for (int c = 0; c < C; ++c) scale[c] = std::exp(logs[c]);
  B.an_escale = pk.add(scale);
  std::vector<float> wfwd;
  if (!invert_small(winv, h.n_split, wfwd)) return fail(MI355TTS_ERR_INVALID, "%s.weight_inv is singular", ic.c_str());
  B.wfwd = pk.add(wfwd);
  WB st, cond, in, rs, end;
  CHECK(r.conv(cp + ".start", H, half, 1, &st));
  B.start = add_conv(pk.f32, st.w, st.b, H, half, 1, ROWS_PLAIN);
  B.t_st = add_col16(pk.f32, st.w, st.b, H, half);
  if (gm.gin()) {  // WN.cond_layer (layers.py:109-113): all blocks' weights side by side for speaker_cond_kernel
    CHECK(r.conv(cp + ".wn.cond_layer", 2 * H * n, gm.gin(), 1, &cond));
    cond_w.insert(cond_w.end(), cond.w, cond.w + (size_t)2 * H * n * gm.gin());
    cond_b.insert(cond_b.end(), cond.b, cond.b + (size_t)2 * H * n);
  }
  for (int j = 0; j < n; ++j) {
    const bool last = j == n - 1;
    const int rsn = last ? H : 2 * H;
    CHECK(r.conv(cp + ".wn.in_layers." + std::to_string(j), 2 * H, H, Kd, &in));
    CHECK(r.conv(cp + ".wn.res_skip_layers." + std::to_string(j), rsn, H, 1, &rs));
    B.in.push_back(add_conv(pk.f32, in.w, in.b, 2 * H, H, Kd, ROWS_PAIR, H));
    add_gate16(pk.f32, B.in.back(), in.w, in.b, H, H, Kd);
    B.rs.push_back(add_plain_conv(pk, rs, rsn, H, 1));
    if (last) B.t_rs = add_col16(pk.f32, rs.w, rs.b, H, H);
    if (gm.f16_ok) {  // the fp16 form of the WaveNet (wn_f16.h)
      B.h_in.push_back(add_wn_gate_h(pk, in.w, in.b, H, Kd));
      if (!last) B.h_rs.push_back(add_wn_rs_h(pk, rs.w, rs.b, H));
    }
  }
  CHECK(r.conv(cp + ".end", C, H, 1, &end));
  B.end = add_conv(pk.f32, end.w, end.b, C, H, 1, ROWS_PAIR, half);
  B.t_end = add_col16(pk.f32, end.w, end.b, C, H);
  B.end_lin = add_conv(pk.f32, end.w, end.b, C, H, 1, ROWS_PLAIN);  // rows in natural order: the forward flow's un-fused form
  gm.blocks.push_back(std::move(B));
  return 0;
}

static int build_glow_model(const mi355tts_glow_hparams& h, BlobReader& r, ModelPacker& pk, GlowModel& gm) {
  gm.hp = h;
  // the fp16 form of the decoder's WaveNets, when the geometry is one its kernel is built for
  gm.f16_why = glow_f16_unsupported(h);
  gm.f16_ok = gm.f16_why.empty();
  CHECK(build_glow_embeddings(h, r, pk, gm));
  if (h.prenet) CHECK(build_glow_prenet(h, r, pk, gm));
  for (int l = 0; l < h.n_layers_enc; ++l) CHECK(build_glow_enc_layer(h, l, r, pk, gm));
  CHECK(build_glow_projections(h, r, pk, gm));
  std::vector<float> cond_w, cond_b;
  for (int b = 0; b < h.n_blocks_dec; ++b) CHECK(build_glow_block(h, b, r, pk, gm, cond_w, cond_b));
  if (gm.gin()) {
    gm.cond_w = pk.add(cond_w);
    gm.cond_b = pk.add(cond_b);
  }
  return 0;
}

// ------------------------------------------------------------------ HiFi-GAN
// the split-bf16 fragments (conv_bf16.h) of a conv with `rows` output rows, where its shape has them
template <class WGet>
static void add_bf16(ModelPacker& pk, DevConv& d, int rows, int Cin, int K, WGet wget) {
  PackedConv16 p = pack_conv_bf16(rows, rows >= 128 ? 4 : rows / 32, Cin, K, wget);
  d.w16_off = ModelPacker::add16(pk.bf16, p.w);
  d.mtiles16 = p.mtiles;
  d.nslab16 = p.nslab;
}

// Narrow stages additionally get the packing of the one-launch MRF kernel (mrf_small.h): ResBlock1 chains with taps
// (3, 7, 11), <= MRF_MAX_STEPS dilation steps and a receptive half-width within the staged halo.
static bool mrf_stage_eligible(const mi355tts_hifigan_hparams& h, int ch) {
  if (h.resblock_type != 1 || h.num_kernels != 3 || (ch != 8 && ch != 16) || h.num_dilations > MRF_MAX_STEPS) return false;
  if (h.resblock_kernel_sizes[0] != 3 || h.resblock_kernel_sizes[1] != 7 || h.resblock_kernel_sizes[2] != 11) return false;
  for (int j = 0; j < h.num_kernels; ++j) {
    int need = 0;
    for (int d = 0; d < h.num_dilations; ++d) {
      if (h.resblock_dilations[j][d] < 1) return false;
      need += (h.resblock_kernel_sizes[j] - 1) / 2 * (h.resblock_dilations[j][d] + 1);
    }
    if (need > MRF_HALO) return false;
  }
  return true;
}

// The convs of one ResBlock step (convs1[d] and convs2[d], or ResBlock2's one conv) in every form their shape gets: the f32
// tiles, split-bf16 fragments when ch is a multiple of 32, fp16 when the model has that mode.  Form by form, not conv by
// conv: that is the order the arenas have always had.
static void pack_res_step(ModelPacker& pk, bool f16_ok, int ch, int k, int nconv, const WB* t, HifiResConv& rc, HResConv& hr) {
  DevConv* c[2] = {&rc.c1, &rc.c2};
  HConvW* hc[2] = {&hr.c1, &hr.c2};
  for (int i = 0; i < nconv; ++i) *c[i] = add_conv(pk.f32, t[i].w, t[i].b, ch, ch, k, ROWS_PLAIN);
  for (int i = 0; i < nconv && ch % 32 == 0; ++i) {
    const float* w = t[i].w;
    add_bf16(pk, *c[i], ch, ch, k, [=](int co, int ci, int kk) { return w[((size_t)co * ch + ci) * k + kk]; });
  }
  for (int i = 0; i < nconv && f16_ok; ++i) *hc[i] = add_conv_h(pk, t[i].w, t[i].b, ch, ch, k);
}

// The MRF small-stage packing of stage tensors t[(j * num_dilations + d) * 2 + conv]: fragments and biases of all 18 convs, and
// the int table [3][MRF_MAX_STEPS][2] fragment offsets | [3][MRF_MAX_STEPS] dilations; C = 8 has a second fragment form
// (mrf8_kernel) with a table of its own.
static void pack_mrf_stage(const mi355tts_hifigan_hparams& h, const std::vector<WB>& t, ModelPacker& pk, MrfStage& ms) {
  const int ch = ms.C;
  ms.ok = true;
  std::vector<float> mrf_w, mrf_w8, mrf_b((size_t)3 * MRF_MAX_STEPS * 2 * 16, 0.f);
  int woff8[3][MRF_MAX_STEPS][2] = {};
  for (int j = 0; j < 3; ++j)
    for (int d = 0; d < h.num_dilations; ++d) {
      const int k = h.resblock_kernel_sizes[j];
      ms.dil[j][d] = h.resblock_dilations[j][d];
      for (int cv = 0; cv < 2; ++cv) {
        const WB& s = t[((size_t)j * h.num_dilations + d) * 2 + cv];
        auto wget = [&](int co, int ci, int kk) { return s.w[((size_t)co * ch + ci) * k + kk]; };
        std::vector<float> f = pack_mrf_conv(ch, k, wget);
        ms.woff[j][d][cv] = (int)mrf_w.size();
        mrf_w.insert(mrf_w.end(), f.begin(), f.end());
        if (ch == 8) {
          std::vector<float> f8 = pack_mrf8_conv(k, wget);
          woff8[j][d][cv] = (int)mrf_w8.size();
          mrf_w8.insert(mrf_w8.end(), f8.begin(), f8.end());
        }
        std::memcpy(&mrf_b[(((size_t)j * MRF_MAX_STEPS + d) * 2 + cv) * 16], s.b, sizeof(float) * ch);
      }
      ms.mac_per_col += 2.0 * ch * ch * k;
    }
  static_assert(sizeof(int) == sizeof(float), "the table rides in the float arena");
  auto add_table = [&](const int (&woff)[3][MRF_MAX_STEPS][2]) {
    int tab[MRF_TAB_INTS] = {};
    for (int j = 0; j < 3; ++j)
      for (int d = 0; d < MRF_MAX_STEPS; ++d) {
        tab[(j * MRF_MAX_STEPS + d) * 2 + 0] = woff[j][d][0];
        tab[(j * MRF_MAX_STEPS + d) * 2 + 1] = woff[j][d][1];
        tab[MRF_TAB_DIL + j * MRF_MAX_STEPS + d] = ms.dil[j][d];
      }
    return pk.add(reinterpret_cast<const float*>(tab), MRF_TAB_INTS);
  };
  ms.w_off = pk.add(mrf_w);
  ms.b_off = pk.add(mrf_b);
  ms.t_off = add_table(ms.woff);
  if (ch == 8) {
    mrf_w8.resize(mrf_w8.size() + 64, 0.f);  // the tap loop's prefetch reads one fragment past the last conv
    ms.w8_off = pk.add(mrf_w8);
    ms.t8_off = add_table(woff8);
  }
}

// upsampler i and the ResBlocks behind it
static int build_hifi_stage(const mi355tts_hifigan_hparams& h, int i, BlobReader& r, ModelPacker& pk, HifiModel& hm) {
  const int cin = h.upsample_initial_channel >> i, ch = cin >> 1;
  const int u = h.upsample_rates[i], ku = h.upsample_kernel_sizes[i];
  hm.hop *= u;
  WB up;
  CHECK(r.conv("ups." + std::to_string(i), ch, cin, ku, &up));  // (a transposed conv's weight is [cin][ch][ku]: as many)
  hm.ups.push_back(add_conv(pk.f32, up.w, up.b, ch, cin, ku, ROWS_UPSAMPLE, u));
  if (hm.f16_ok) hm.h_ups.push_back(add_ups_h(pk, up.w, up.b, ch, cin, u));
  if (cin % 32 == 0 && (ch * u) % 32 == 0 && ku / u == 2) add_bf16(pk, hm.ups.back(), ch * u, cin, 2, PolyphaseW{up.w, ch, ku, u});
  const int nconv = h.resblock_type == 1 ? 2 : 1;
  std::vector<WB> t((size_t)h.num_kernels * h.num_dilations * 2);
  hm.rb[i].resize(h.num_kernels);
  if (hm.f16_ok) hm.h_rb[i].resize(h.num_kernels);
  for (int j = 0; j < h.num_kernels; ++j) {
    const std::string rb = "resblocks." + std::to_string(i * h.num_kernels + j);
    const int k = h.resblock_kernel_sizes[j];
    for (int d = 0; d < h.num_dilations; ++d) {
      WB* s = &t[((size_t)j * h.num_dilations + d) * 2];
      if (nconv == 2) {
        CHECK(r.conv(rb + ".convs1." + std::to_string(d), ch, ch, k, &s[0]));
        CHECK(r.conv(rb + ".convs2." + std::to_string(d), ch, ch, k, &s[1]));
      } else {
        CHECK(r.conv(rb + ".convs." + std::to_string(d), ch, ch, k, &s[0]));
      }
      HifiResConv rc;
      HResConv hr;
      rc.dil = h.resblock_dilations[j][d];
      pack_res_step(pk, hm.f16_ok, ch, k, nconv, s, rc, hr);
      hm.rb[i][j].push_back(rc);
      if (hm.f16_ok) hm.h_rb[i][j].push_back(hr);
    }
  }
  MrfStage ms;
  ms.C = ch;
  ms.nsteps = h.num_dilations;
  if (mrf_stage_eligible(h, ch)) pack_mrf_stage(h, t, pk, ms);
  hm.mrf.push_back(ms);
  return 0;
}

static int build_hifi_model(const mi355tts_hifigan_hparams& h, BlobReader& r, ModelPacker& pk, HifiModel& hm) {
  hm.hp = h;
  // the native fp16 mode's packing of every conv (hifigan_f16.h), when the geometry is one its tiles cover
  hm.f16_why = hifi_f16_unsupported(h);
  hm.f16_ok = hm.f16_why.empty();
  const int C0 = h.upsample_initial_channel, Cpost = C0 >> h.num_upsamples;
  WB pre, post;
  CHECK(r.conv("conv_pre", C0, h.num_mels, 7, &pre));
  hm.pre = add_conv(pk.f32, pre.w, pre.b, C0, h.num_mels, 7, ROWS_PLAIN);
  if (hm.f16_ok) hm.h_pre = add_conv_h(pk, pre.w, pre.b, C0, h.num_mels, 7);
  hm.hop = 1;
  hm.rb.resize(h.num_upsamples);
  if (hm.f16_ok) hm.h_rb.resize(h.num_upsamples);
  for (int i = 0; i < h.num_upsamples; ++i) CHECK(build_hifi_stage(h, i, r, pk, hm));
  CHECK(r.conv("conv_post", 1, Cpost, 7, &post));
  hm.post = add_conv(pk.f32, post.w, post.b, 1, Cpost, 7, ROWS_PLAIN);
  hm.post_w_off = pk.add(post.w, (size_t)Cpost * 7);  // raw [C][7] + bias for post_conv_kernel (voc_out.h)
  hm.post_b_off = pk.add(post.b, 1);
  hm.post_C = Cpost;
  return 0;
}
