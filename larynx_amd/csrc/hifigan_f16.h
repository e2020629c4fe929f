// mi355tts host runtime — the native fp16 vocoder (MI355TTS_PRECISION_F16): what the reference's `half` switch is, `.half()` on
// the whole HiFi-GAN generator (larynx/hifi_gan.py:96-97; hifi_gan/models.py:91-98, 136-141, 186-202).  Weight packing at load,
// the tile choice, the plans and the launches of conv_f16.h's kernels; the layer schedule is hifigan_body_f16 in hifigan_forward.h.  Every layer of the generator runs in this mode: conv_pre,
// the upsamplers, every ResBlock conv of every stage (wide and narrow) and conv_post read and write fp16 planes; the
// waveform leaves conv_post's tanh in f32 (the reference casts its half output to float there, larynx/hifi_gan.py:160-166).
// (one translation unit: included once by mi355tts.hip, after host_launch.h)
#pragma once

// ------------------------------------------------------------------ geometry the fp16 tiles cover
static int f16_halo(int K) {
  switch (K) {
    case 3: return ConvHalo<3>::v;
    case 5: return ConvHalo<5>::v;
    case 7: return ConvHalo<7>::v;
    case 11: return ConvHalo<11>::v;
    default: return -1;
  }
}
// "" when the model can run in fp16, else what stands in the way (mi355tts_model_set_precision reports it)
static std::string hifi_f16_unsupported(const mi355tts_hifigan_hparams& h) {
  const int C0 = h.upsample_initial_channel;
  if (h.num_kernels < 2 || h.num_kernels > 3) return "the fp16 schedule needs 2 or 3 ResBlock chains per stage";
  for (int i = 0; i < h.num_upsamples; ++i) {
    const int cin = C0 >> i, cout = C0 >> (i + 1);
    if ((cin % 8) || (cout % 8) || cout < 8) return "channel counts must be multiples of 8 (16-byte octet units)";
    if (h.upsample_kernel_sizes[i] != 2 * h.upsample_rates[i]) return "upsampler kernel must be twice its stride (two polyphase taps)";
  }
  if ((C0 >> h.num_upsamples) > 64) return "more than 64 channels into conv_post";
  for (int j = 0; j < h.num_kernels; ++j) {
    const int K = h.resblock_kernel_sizes[j];
    const int halo = f16_halo(K);
    if (halo < 0) return "ResBlock kernel size not one of 3, 5, 7, 11";
    for (int d = 0; d < h.num_dilations; ++d)
      if (h.resblock_dilations[j][d] < 1 || h.resblock_dilations[j][d] * (K - 1) > halo) return "ResBlock dilation beyond the staged halo";
  }
  return "";
}

// one conv into the fp16 arena; its f32 bias rides in the model's float arena
static HConvW add_h(ModelPacker& pk, const PackedConvH& p, int Cin) {
  HConvW d;
  d.w_off = ModelPacker::add16(pk.f16, p.w);
  d.b_off = pk.add(p.bias);
  d.mtiles = p.mtiles;
  d.nslab = p.nslab;
  d.K = p.K;
  d.rows = p.rows;
  d.Cin = Cin;
  return d;
}
// a plain conv w[Cout][Cin][K]
static HConvW add_conv_h(ModelPacker& pk, const float* w, const float* bias, int Cout, int Cin, int K) {
  return add_h(pk, pack_conv_f16(
                    Cout, 4, Cin, K, 64, [&](int v, int ci, int k) { return w[((size_t)v * Cin + ci) * K + k]; }, [&](int v) { return bias[v]; },
                    bias != nullptr),
                Cin);
}
// ConvTranspose1d(Cin, Cout, 2 u, stride u, padding u / 2) in polyphase form: virtual row v = r * Cout + co (phase-major), two
// taps over q, tap k reads x[q + k - 1] and carries Wt[ci][co][(1 - k) u + r]  (see PolyphaseW for the derivation).  Not
// PolyphaseW's row order: the fp16 planes hold 8 channels per 16-byte unit, so a lane's 4 consecutive rows must be 4
// consecutive channels of ONE output sample (conv_f16.h, EPI_UPSAMPLE); the f32 and split-bf16 tiles write rows of time and
// keep a channel's u phases together.
static HConvW add_ups_h(ModelPacker& pk, const float* wt, const float* bias, int Cout, int Cin, int u) {
  const int Ku = 2 * u;
  return add_h(pk, pack_conv_f16(
                    Cout * u, 4, Cin, 2, 64,
                    [&](int v, int ci, int k) {
                      const int r = v / Cout, co = v % Cout, m = 1 - k;
                      return wt[((size_t)ci * Cout + co) * Ku + m * u + r];
                    },
                    [&](int v) { return bias[v % Cout]; }, bias != nullptr),
                Cin);
}
// ---- the WaveNets of GlowTTS' coupling blocks for wn_f16_kernel (wn_f16.h)
static std::string glow_f16_unsupported(const mi355tts_glow_hparams& h) {
  if (h.hidden_channels != 192 && h.hidden_channels != 32) return "hidden_channels other than 192 (32)";
  if (h.kernel_size_dec != 5) return "kernel_size_dec other than 5";
  if (h.dilation_rate != 1) return "dilated WaveNet layers";
  if (h.n_speakers > 1) return "speaker conditioning";
  if (h.n_block_layers < 1 || h.n_block_layers > WN_MAX_LAYERS || 4 * h.n_block_layers >= WN_W) return "n_block_layers";
  return "";
}
// in_layers[j]: w [2H][H][K]; virtual 32-row tile p = the tanh rows of channels 16 p .. 16 p + 15, then their sigmoid rows
static HConvW add_wn_gate_h(ModelPacker& pk, const float* w, const float* bias, int H, int K) {
  auto row_of = [H](int v) {
    const int p = v / 32, i = v % 32, c = 16 * p + (i & 15);
    return i < 16 ? c : H + c;
  };
  return add_h(pk, pack_conv_f16(
                    2 * H, 1, H, K, 32, [&](int v, int ci, int k) { return w[((size_t)row_of(v) * H + ci) * K + k]; },
                    [&](int v) { return bias[row_of(v)]; }, true),
                H);
}
// res_skip_layers[j] (j < n - 1): w [2H][H][1], rows in natural order [res | skip]
static HConvW add_wn_rs_h(ModelPacker& pk, const float* w, const float* bias, int H) {
  return add_h(pk, pack_conv_f16(
                    2 * H, 1, H, 1, 32, [&](int v, int ci, int) { return w[(size_t)v * H + ci]; }, [&](int v) { return bias[v]; }, true),
                H);
}

// ------------------------------------------------------------------ tiles
// Three tile shapes (all 256 threads, 32-channel staged chunks), chosen by the conv's output rows and input channels:
//   WIDE : 2 x 2 waves of 64 rows x 64 columns — 128 rows x 128 columns per workgroup, the three-chunk ring (any Cin)
//   MID  : 1 x 4 waves of 64 x 64              —  64 rows x 256 columns, Cin <= 64: both chunks staged in the prologue
//   SLIM : 1 x 4 waves of 32 x 64              —  32 rows x 256 columns, Cin <= 32: the one chunk
enum HTile { HT_WIDE = 0, HT_MID, HT_SLIM };
static int h_tile_for(int rows, int Cin) { return (rows <= 32 && Cin <= 32) ? HT_SLIM : (rows < 128 && Cin <= 64) ? HT_MID : HT_WIDE; }
// template arguments MB, NB, WM, WN of each shape (a tile is 32 MB WM rows x 32 NB WN columns), the depth of its chunk ring and
// the waves per SIMD the fused pair kernel asks for
struct HTileCfg {
  int MB, NB, WM, WN, RING, PAIR_MINW;
};
constexpr HTileCfg H_TILES[3] = {{2, 2, 2, 2, 3, 3}, {2, 2, 1, 4, 2, 3}, {1, 2, 1, 4, 1, 4}};
constexpr int H_CH = 32;
static void h_tile_dims(int t, int& trows, int& tcols) {
  trows = 32 * H_TILES[t].MB * H_TILES[t].WM;
  tcols = 32 * H_TILES[t].NB * H_TILES[t].WN;
}
// f(tile configuration as a compile-time index); < 0 with the error set for a tile that does not exist
template <class F>
static int h_tile_dispatch(int tile, F&& f) {
  return switch_const<HT_WIDE, HT_MID, HT_SLIM>(tile, f) ? 0 : fail(MI355TTS_ERR_INVALID, "internal: fp16 tile %d", tile);
}

struct HPlan {
  HConvArgs a;
  int K = 0, tile = 0, epi = EPI_LINEAR;
  bool mrf = false;
  dim3 grid;
  int gx = 0, gy = 0;
  double flop = 0;
};

template <int K, int EPI, bool MRF>
static int launch_f16_k(const HPlan& p, hipStream_t s) {
  return h_tile_dispatch(p.tile, [&](auto tile) {
    constexpr HTileCfg t = H_TILES[decltype(tile)::value];
    hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_f16_kernel<K, t.MB, t.NB, t.WM, t.WN, ConvHalo<K>::v, H_CH, EPI, MRF, t.RING>), p.grid, dim3(256), 0, s, p.a);
  });
}
static int run_plan_f16(mi355tts_ctx* ctx, Worker* w, const HPlan& p, int cls, hipStream_t s) {
  ProfScope ps(ctx, w, cls, p.flop, s);
  ps.kernel(KN_CONV_F16, p.a.rows);
  if (p.epi == EPI_UPSAMPLE) return p.mrf ? launch_f16_k<2, EPI_UPSAMPLE, true>(p, s) : launch_f16_k<2, EPI_UPSAMPLE, false>(p, s);
  int rc = 0;
  if (!switch_const<3, 5, 7, 11>(p.K, [&](auto k) { rc = launch_f16_k<decltype(k)::value, EPI_LINEAR, false>(p, s); }))
    rc = fail(MI355TTS_ERR_INVALID, "internal: fp16 conv with %d taps", p.K);
  return rc;
}

// The same-geometry convs of a step's three chains in ONE launch (members longest first).  Returns 0 = launched, 1 = this tap
// set has no grouped kernel (the caller launches the members one by one), < 0 = error.
static int run_group_f16(mi355tts_ctx* ctx, Worker* w, const HPlan* p, int n, int B, hipStream_t s) {
  if (n != 3) return 1;
  const int K[3] = {p[0].K, p[1].K, p[2].K}, tiles[3] = {p[0].gx * p[0].gy, p[1].gx * p[1].gy, p[2].gx * p[2].gy};
  const GroupLayout lay = group_layout(K, tiles);
  if (!lay.k1173 && !lay.k753) return 1;
  if (p[0].tile != p[1].tile || p[0].tile != p[2].tile) return 1;
  HConvGroupArgs g;
  std::memset(&g, 0, sizeof(g));
  double flop = 0;
  for (int m = 0; m < 3; ++m) {
    const HPlan& q = p[lay.ord[m]];
    g.c[m] = q.a;
    g.gx[m] = q.gx;
    g.gy[m] = q.gy;
    flop += q.flop;
  }
  std::copy(lay.off, lay.off + 4, g.off);
  ProfScope ps(ctx, w, KC_RESBLOCK, flop, s);
  ps.kernel(KN_CONV_F16_GROUP, p[0].a.rows);
  const dim3 grid(g.off[3], 1, B);
  int rc = 0;
  switch_taps(lay, [&](auto k0, auto k1, auto k2) {
    rc = h_tile_dispatch(p[0].tile, [&](auto tile) {
      constexpr int K0 = decltype(k0)::value, K1 = decltype(k1)::value, K2 = decltype(k2)::value;
      constexpr HTileCfg t = H_TILES[decltype(tile)::value];
      hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_f16_group_kernel<K0, K1, K2, t.MB, t.NB, t.WM, t.WN, ConvHalo<K0>::v, ConvHalo<K1>::v, ConvHalo<K2>::v, H_CH, t.RING>),
                         grid, dim3(256), 0, s, g);
    });
  });
  return rc;
}

// ---- fused ResBlock1 steps (pair_f16.h): conv1 + conv2 of a dilation step of the three chains in ONE launch.  A workgroup owns
// all channels of its columns, so the tile is chosen by the channel count: C <= 32 SLIM, C <= 64 MID, C <= 128 WIDE.
struct HPairPlan {
  HPairArgs a;
  int K = 0;
  double flop = 0;
};
static int h_pair_tile(int C) { return C <= 32 ? HT_SLIM : C <= 64 ? HT_MID : C <= 128 ? HT_WIDE : -1; }
// Returns 0 = launched, 1 = not covered (the caller runs conv1 and conv2 as two grouped launches), < 0 = error.
static int run_pair_group_f16(mi355tts_ctx* ctx, Worker* w, const HPairPlan* p, int n, int C, int B, int Lmax, hipStream_t s) {
  if (n != 3) return 1;
  const int tile = h_pair_tile(C);
  if (tile < 0) return 1;
  int tr, tc;
  h_tile_dims(tile, tr, tc);
  int K[3], gx[3];
  for (int j = 0; j < 3; ++j) {
    const int to = tc - (p[j].K - 1);  // output columns of a tile
    K[j] = p[j].K;
    gx[j] = (Lmax + to - 1) / to;
  }
  const GroupLayout lay = group_layout(K, gx);
  if (!lay.k1173) return 1;
  HPairGroupArgs g;
  std::memset(&g, 0, sizeof(g));
  g.n = 3;
  double flop = 0;
  for (int m = 0; m < 3; ++m) {
    const HPairPlan& q = p[lay.ord[m]];
    g.p[m] = q.a;
    g.gx[m] = gx[lay.ord[m]];
    flop += q.flop;
  }
  std::copy(lay.off, lay.off + 4, g.off);
  ProfScope ps(ctx, w, KC_RESBLOCK, flop, s);
  ps.kernel(KN_PAIR_F16_GROUP, C);
  return h_tile_dispatch(tile, [&](auto ti) {
    constexpr HTileCfg t = H_TILES[decltype(ti)::value];
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_f16_group_kernel<11, 7, 3, t.MB, t.NB, t.WM, t.WN, ConvHalo<11>::v, ConvHalo<7>::v, ConvHalo<3>::v, H_CH, t.RING, t.PAIR_MINW>),
                       dim3(g.off[3], 1, B), dim3(256), 0, s, g);
  });
}

// lengths: one row with a host-known length takes it as a launch constant (no dependent load in every workgroup's prologue)
static void h_set_lengths(HConvArgs& a, int B, const int* d_frames, int host_len, int in_mul, int out_mul) {
  const RowLen in = row_len(B, host_len, d_frames, in_mul), out = row_len(B, host_len, d_frames, out_mul);
  a.in_len = in.len; a.in_const = in.len_const;
  a.out_len = out.len; a.out_const = out.len_const;
  a.in_mul = in_mul;
  a.out_mul = out_mul;
}
static HPlan plan_f16(const HConvW& c, HConvArgs a, int epi, int B, int n_max, double flop) {
  HPlan p;
  a.w = c.w;
  a.bias = c.bias;
  a.nslab = c.nslab;
  a.Cin = c.Cin;
  a.rows = c.rows;
  p.a = a;
  p.K = c.K;
  p.epi = epi;
  p.tile = h_tile_for(c.rows, c.Cin);
  int tr, tc;
  h_tile_dims(p.tile, tr, tc);
  p.gx = (n_max + tc - 1) / tc;
  p.gy = (c.rows + tr - 1) / tr;
  p.grid = dim3(p.gx, p.gy, B);
  p.flop = flop;
  return p;
}
