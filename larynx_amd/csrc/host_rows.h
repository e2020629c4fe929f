// mi355tts host runtime — the rows of a call and their delivery: the row view of a call's outputs (OutRow / OutRows), where host
// outputs wait in the pinned staging (Staging), the delivery itself (zero_outputs, stage_rows, scatter_rows, deliver_rows), which
// the vocoders, Griffin-Lim and the delivery stages share, and WaveCall: the frame of a wave-in / wave-out call (resampling,
// loudness, the limiter).
// (one translation unit: included once by mi355tts.hip, after host_call.h)
#pragma once

// ------------------------------------------------------------------ the rows of a call
struct VocRow {  // one row's destinations when the rows of a call belong to different callers (host_join.h)
  float* wav_f32 = nullptr;
  int16_t* wav_i16 = nullptr;
  int64_t wav_ld = 0;
  int pad_before = 0, pad_after = 0;
};
// One output row as the host-side code sees it: [pad_before zeros][n samples][zeros up to ld]; the int16 row travels with its
// pauses (the kernels write them), n + pad_before + pad_after values.  A null pointer = no such output.
struct OutRow {
  float* f32;
  int16_t* i16;
  int64_t ld;
  size_t pad_before, pad_after, n;
};
// The rows of a call: every caller's own destinations (`rows`: row b travels with its OWN length, its caller's buffer is sized for
// its own frame count), or one [B][ld] buffer per form (every row travels with the longest row's `n` samples; the kernels zeroed
// what lies behind a short row's).  An accessor, not an array: a whole-batch call may have more than VOC_MAX_ROWS rows.
struct OutRows {
  const VocRow* rows;
  const int32_t* frames;  // with `rows`: samples of row b = frames[b] * hop
  int hop;
  OutRow all;  // without `rows`: row 0; row b lies b * ld behind it
  OutRow operator()(int b) const {
    if (rows) return {rows[b].wav_f32, rows[b].wav_i16, rows[b].wav_ld, (size_t)rows[b].pad_before, (size_t)rows[b].pad_after, (size_t)frames[b] * hop};
    OutRow r = all;
    if (r.f32) r.f32 += (size_t)b * r.ld;
    if (r.i16) r.i16 += (size_t)b * r.ld;
    return r;
  }
};

// Where a call's host outputs wait in the worker's pinned staging, from byte `at` of it: the float rows [B][f_ld], the int16
// rows [B][i_ld], then one extra block.  Sized before the call's first launch (CallFrame::reserve), read by deliver_rows.
struct Staging {
  size_t at = 0, f32_b = 0, i16_b = 0, extra_b = 0, f_ld = 0, i_ld = 0;
  size_t end() const { return at + f32_b + i16_b + extra_b; }
};
static Staging host_staging(int B, bool f32, size_t f_ld, bool i16, size_t i_ld, size_t at = 0, size_t extra_b = 0) {
  return {at, f32 ? sizeof(float) * (size_t)B * f_ld : 0, i16 ? sizeof(short) * (size_t)B * i_ld : 0, extra_b, f_ld, i_ld};
}

// ------------------------------------------------------------------ delivery
// fills and copies into the caller's rows: in host memory, or queued on the stream for device memory.  Empty pieces are skipped.
struct RowWriter {
  bool dev;
  hipStream_t s;
  template <class T>
  int zero(T* dst, size_t n) const {
    if (n && dev) HIPCHECK(hipMemsetAsync(dst, 0, sizeof(T) * n, s));
    if (n && !dev) std::memset(dst, 0, sizeof(T) * n);
    return 0;
  }
  template <class T>
  int copy(T* dst, const T* src, size_t n) const {
    if (n && dev) HIPCHECK(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToDevice, s));
    if (n && !dev) std::memcpy(dst, src, sizeof(T) * n);
    return 0;
  }
};

// an empty call: every output row all zeros (whole-batch rows lie back to back: one fill per form); ends the frame's work
static int zero_outputs(CallFrame& f, const OutRows& rows, int B, bool dev) {
  const RowWriter wr{dev, f.s};
  const int nfill = rows.rows ? B : 1;
  const size_t span = rows.rows ? 1 : (size_t)B;
  for (int b = 0; b < nfill; ++b) {
    const OutRow r = rows(b);
    if (r.f32) CHECK(wr.zero(r.f32, span * (size_t)r.ld));
    if (r.i16) CHECK(wr.zero(r.i16, span * (size_t)r.ld));
  }
  if (dev) HIPCHECK(f.wait());
  f.done = true;
  return 0;
}

// finished rows in staging memory: float rows [B][f_ld] of samples alone, int16 rows [B][i_ld] with their pauses
struct WavRows {
  float* f32;
  size_t f_ld;
  short* i16;
  size_t i_ld;
};
// staging rows -> the caller's: pause | samples | zeros up to the row stride
static int scatter_rows(const OutRows& rows, int B, const WavRows& src, const RowWriter& wr) {
  for (int b = 0; b < B; ++b) {
    const OutRow r = rows(b);
    const size_t rl = r.pad_before + r.n + r.pad_after;
    if (r.f32) {
      float* dst = r.f32;
      CHECK(wr.zero(dst, r.pad_before));
      CHECK(wr.copy(dst + r.pad_before, src.f32 + (size_t)b * src.f_ld, r.n));
      CHECK(wr.zero(dst + r.pad_before + r.n, (size_t)r.ld - r.pad_before - r.n));
    }
    if (r.i16) {
      int16_t* dst = r.i16;
      CHECK(wr.copy(dst, src.i16 + (size_t)b * src.i_ld, rl));
      CHECK(wr.zero(dst + rl, (size_t)r.ld - rl));
    }
  }
  return 0;
}
// device rows -> pinned rows of the same shape (async DMA): the part of every row that its caller receives
static int stage_rows(const OutRows& rows, int B, const WavRows& dev, const WavRows& pin, hipStream_t s) {
  for (int b = 0; b < B; ++b) {
    const OutRow r = rows(b);
    if (r.f32 && r.n) HIPCHECK(hipMemcpyAsync(pin.f32 + (size_t)b * pin.f_ld, dev.f32 + (size_t)b * dev.f_ld, sizeof(float) * r.n, hipMemcpyDeviceToHost, s));
    if (r.i16) HIPCHECK(hipMemcpyAsync(pin.i16 + (size_t)b * pin.i_ld, dev.i16 + (size_t)b * dev.i_ld, sizeof(short) * (r.n + r.pad_before + r.pad_after), hipMemcpyDeviceToHost, s));
  }
  return 0;
}

// Host delivery: device rows -> the pinned staging `st` describes (async DMA) -> the end of the frame's device work -> the
// caller's (pageable) rows.  `block`: the staging keeps the device rows' strides and each form goes in ONE copy; else row by
// row, the part its caller receives.  `extra_src` (device, st.extra_b bytes) rides along to `extra_dst`.
static int deliver_rows(CallFrame& f, const OutRows& rows, int B, const WavRows& dev, const Staging& st, bool block, void* extra_dst = nullptr,
                        const void* extra_src = nullptr) {
  char* pf = f.w->pinned_out + st.at;
  char* pi = pf + st.f32_b;
  char* px = pi + st.i16_b;
  const WavRows pin = {(float*)pf, st.f_ld, (short*)pi, st.i_ld};
  if (!block) CHECK(stage_rows(rows, B, dev, pin, f.s));
  if (block && st.f32_b) HIPCHECK(hipMemcpyAsync(pf, dev.f32, st.f32_b, hipMemcpyDeviceToHost, f.s));
  if (block && st.i16_b) HIPCHECK(hipMemcpyAsync(pi, dev.i16, st.i16_b, hipMemcpyDeviceToHost, f.s));
  if (st.extra_b) HIPCHECK(hipMemcpyAsync(px, extra_src, st.extra_b, hipMemcpyDeviceToHost, f.s));
  CHECK(f.finish());
  CHECK(scatter_rows(rows, B, pin, RowWriter{false, f.s}));
  if (st.extra_b) std::memcpy(extra_dst, px, st.extra_b);
  return 0;
}

// ------------------------------------------------------------------ a wave-in / wave-out call
// What the delivery stages share around their launches: rows of samples in (WaveIn), [B][out_ld] rows out in either form or both,
// optionally a SIDE PLANE [B][in_ld] of floats (N values | zeros per row) and RESULTS (a few floats per row, each into a nullable
// [B] array).  Host outputs travel workspace -> pinned staging -> the caller's rows; device outputs are written in place by the
// stage's kernels, zero tails included.  A stage runs: check_args, its own scalar checks, find_model, in.check, check_out, open,
// [no samples: empty], carve -> its own workspace takes -> reserve, its launches (in.bind; d_y / d_pcm / d_side / d_res), end.
struct WaveCall {
  WaveIn in;
  float* out_f32;
  int16_t* out_i16;
  int64_t out_ld;
  bool out_dev;
  CallFrame f;
  // check_out / open: the longest output row, the caller's rows, its side plane and result arrays
  long long Nout = 0;
  OutRows rows = {};
  float *side = nullptr, *res_out[4] = {};
  int nres = 0;
  // carve: the workspace stride of host-bound output rows, the takes, the staging (rows and results, then the side plane)
  size_t Nld = 0, o_y = 0, o_pcm = 0, o_side = 0, o_res = 0, side_host = 0;
  Staging st;
  // a stage's own bytes of pinned staging behind all of that (at extra_at()), set before reserve: what else it sends or receives
  size_t extra_host = 0;
  size_t extra_at() const { return st.end() + side_host; }
  // reserve: what the kernels write, and at which row strides
  float *d_y = nullptr, *d_side = nullptr, *d_res = nullptr;
  short* d_pcm = nullptr;
  long long ld = 0, side_ld = 0;

  WaveCall(mi355tts_ctx* ctx, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B, int64_t in_ld, float* of32,
           int16_t* oi16, int64_t old, uint32_t flags)
      : in{in_f32, in_i16, samples, B, in_ld, (flags & MI355TTS_IN_DEVICE) != 0}, out_f32(of32), out_i16(oi16), out_ld(old),
        out_dev((flags & MI355TTS_OUT_DEVICE) != 0), f(ctx) {}

  int check_args() const {
    if (!f.ctx || !in.samples) return fail(MI355TTS_ERR_INVALID, "null argument");
    if ((in.f32 != nullptr) == (in.i16 != nullptr)) return fail(MI355TTS_ERR_INVALID, "exactly one of in_f32 / in_i16 must be given");
    if (in.B <= 0 || in.ld < 0) return fail(MI355TTS_ERR_INVALID, "empty batch or negative in_ld");
    return 0;
  }
  int check_out(long long longest) {
    Nout = longest;
    if ((out_f32 || out_i16) && out_ld < Nout) return fail(MI355TTS_ERR_INVALID, "out_ld %lld < %lld samples of the longest row", (long long)out_ld, Nout);
    return 0;
  }
  int open(float* side_plane = nullptr, std::initializer_list<float*> results = {}) {
    side = side_plane;
    for (float* r : results) res_out[nres++] = r;
    rows = {nullptr, nullptr, 0, {out_f32, out_i16, out_ld, 0, 0, (size_t)Nout}};
    return f.open();
  }
  // no sample in any output row: the stage's per-row results, a zero side plane, every output row all zeros
  int empty(std::initializer_list<float> defaults) {
    int k = 0;
    for (float d : defaults) {
      if (res_out[k]) std::fill_n(res_out[k], in.B, d);
      ++k;
    }
    if (side) CHECK((RowWriter{out_dev, f.s}).zero(side, (size_t)in.B * (size_t)in.ld));
    return zero_outputs(f, rows, in.B, out_dev);
  }
  // the input, then what travels to the host: rows, results and the side plane (a device side plane is written in place)
  Carver carve() {
    const size_t B = (size_t)in.B;
    Nld = (size_t)((Nout + 7) & ~7LL);
    side_host = side && !out_dev ? sizeof(float) * B * in.Nld : 0;
    Carver cv;
    in.carve(cv);
    o_y = cv.take(out_f32 && !out_dev ? sizeof(float) * B * Nld : 0);
    o_pcm = cv.take(out_i16 && !out_dev ? sizeof(short) * B * Nld : 0);
    o_side = cv.take(side_host);
    o_res = cv.take(sizeof(float) * nres * B);
    // host outputs wait in the pinned staging behind the staged input: the delivered rows and the results, then the side plane
    st = host_staging(in.B, out_f32 && !out_dev, Nld, out_i16 && !out_dev, Nld, in.bytes, sizeof(float) * nres * B);
    return cv;
  }
  // the workspace `cv` ends at and the staging; queues the input's upload
  int reserve(const Carver& cv) {
    CHECK(f.reserve(cv.pos, st.end() + side_host + extra_host));
    char* base = f.w->arena;
    CHECK(in.upload(f, f.w->pinned));
    ld = out_dev ? (long long)out_ld : (long long)Nld;
    d_y = !out_f32 ? nullptr : out_dev ? out_f32 : (float*)(base + o_y);
    d_pcm = !out_i16 ? nullptr : out_dev ? (short*)out_i16 : (short*)(base + o_pcm);
    d_side = !side ? nullptr : out_dev ? side : (float*)(base + o_side);
    side_ld = out_dev ? (long long)in.ld : (long long)in.Nld;
    d_res = (float*)(base + o_res);
    return 0;
  }
  // behind the last launch: device outputs with no results just end the frame's work; else the host's share is delivered
  int end() {
    if (out_dev && !nres) return f.finish();
    const int B = in.B;
    char* const p_side = f.w->pinned_out + st.end();
    if (side_host) HIPCHECK(hipMemcpyAsync(p_side, d_side, side_host, hipMemcpyDeviceToHost, f.s));
    std::vector<float> res((size_t)nres * B);
    // (with device outputs the staging holds no rows: the results alone travel, and scatter_rows finds nothing to write)
    const OutRows host_rows = out_dev ? OutRows{nullptr, nullptr, 0, {nullptr, nullptr, 0, 0, 0, 0}} : rows;
    CHECK(deliver_rows(f, host_rows, B, WavRows{d_y, Nld, d_pcm, Nld}, st, true, res.data(), d_res));
    for (int b = 0; b < B; ++b) {
      for (int k = 0; k < nres; ++k)
        if (res_out[k]) res_out[k][b] = res[(size_t)nres * b + k];
      if (side_host) {
        float* dst = side + (size_t)b * (size_t)in.ld;
        std::memcpy(dst, p_side + sizeof(float) * (size_t)b * in.Nld, sizeof(float) * (size_t)in.samples[b]);
        std::memset(dst + in.samples[b], 0, sizeof(float) * ((size_t)in.ld - (size_t)in.samples[b]));
      }
    }
    return 0;
  }
};
