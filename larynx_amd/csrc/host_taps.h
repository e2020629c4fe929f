// mi355tts host runtime — the test seam: the planes of one tapped call
// (one translation unit: included once by mi355tts.hip, behind host_context.h and ahead of both forward files)
// mi355tts_hifigan_infer_taps / mi355tts_glow_infer_taps keep a device copy of every plane their schedule wrote, taken in stream
// order right behind the launch that wrote it: the schedules reuse their planes, so a copy at the end of the call would be too
// late.  The store is owned by the context (mi355tts_ctx::voc_taps) and replaced by the next such call of either kind.  The passes
// (VocPass, GlowPass) hold a null `taps` pointer in every other call and test it first: with ProfScope::kernel's test of `kn_out`,
// all a plain call pays for the seam.
#pragma once

struct VocTap {
  std::string name;
  int kn = -1;       // the kernel name the writing launch was counted under (KName; -1: none)
  bool f16 = false;  // fp16 octet planes [B][ch / 8][ld][8]; else f32 [B][ch][ld]
  int B = 0, ch = 0, ld = 0;
  std::vector<int> len;  // valid columns per row
  void* dev = nullptr;
  size_t bytes = 0;
};
struct VocTaps {
  static constexpr size_t MAX_BYTES = (size_t)256 << 20;
  std::vector<VocTap> taps;
  size_t bytes = 0;
  int last_kn = -1;  // ProfScope::kernel writes the running launch's name here (ProfLane::kn_out)
  VocTaps() = default;
  VocTaps(const VocTaps&) = delete;
  ~VocTaps() {
    for (auto& t : taps)
      if (t.dev) hipFree(t.dev);
  }

  // A copy of plane `x` — `ch` channels at row stride `ld`, fp16 octet planes or f32 rows, `len[b]` valid columns in row b — queued
  // on stream `s` behind whatever wrote it, and filed under the kernel name that launch was counted under ("-": a launch without
  // one).  `same_launch`: a further plane of the launch that wrote the previous tap.
  int add(hipStream_t s, const std::string& name, const void* x, bool f16, int B, int ch, int ld, const int* len, bool same_launch) {
    VocTap t;
    t.name = name;
    t.kn = same_launch && !taps.empty() ? taps.back().kn : last_kn;
    last_kn = -1;  // (most small GlowTTS launches are counted under no name: the next tap must not inherit this one's)
    t.f16 = f16;
    t.B = B;
    t.ch = ch;
    t.ld = ld;
    for (int b = 0; b < B; ++b) t.len.push_back(std::min(len[b], ld));
    t.bytes = f16 ? (size_t)B * (size_t)((ch + 7) / 8) * (size_t)ld * 16 : sizeof(float) * (size_t)B * (size_t)ch * (size_t)ld;
    if (bytes + t.bytes > MAX_BYTES)
      return fail(MI355TTS_ERR_NOMEM, "the planes of this call exceed %zu MB of tap copies (at '%s'): fewer frames or rows", MAX_BYTES >> 20, name.c_str());
    HIPCHECK(hipMalloc(&t.dev, t.bytes));
    bytes += t.bytes;
    taps.push_back(t);  // (owned from here on: ~VocTaps frees it)
    HIPCHECK(hipMemcpyAsync(t.dev, x, t.bytes, hipMemcpyDeviceToDevice, s));
    return 0;
  }

  // [{"name": "up0", "channels": 64, "ld": 140, "len": [140, 18], "f16": 1, "kernel": "conv_f16_kernel"}, ...] in launch order
  std::string json() const {
    std::string s = "[";
    for (size_t i = 0; i < taps.size(); ++i) {
      const VocTap& t = taps[i];
      char tmp[256];
      std::snprintf(tmp, sizeof(tmp), "%s{\"name\": \"%s\", \"channels\": %d, \"ld\": %d, \"len\": [", i ? ", " : "", t.name.c_str(), t.ch, t.ld);
      s += tmp;
      for (size_t b = 0; b < t.len.size(); ++b) s += (b ? ", " : "") + std::to_string(t.len[b]);
      std::snprintf(tmp, sizeof(tmp), "], \"f16\": %d, \"kernel\": \"%s\"}", t.f16 ? 1 : 0, t.kn >= 0 && t.kn < KN_COUNT ? kname_name[t.kn] : "-");
      s += tmp;
    }
    return s + "]";
  }
};

static std::string tap_name(const char* fmt, ...) {
  char tmp[64];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(tmp, sizeof(tmp), fmt, ap);
  va_end(ap);
  return tmp;
}

// A tapped call learns its launches' names through the worker (`taps` null: a plain call, nothing to learn); the worker forgets
// the address on every way out.
struct TapNames {
  ProfLane* w;
  TapNames(ProfLane* w_, VocTaps* taps) : w(w_) {
    if (taps) w->kn_out = &taps->last_kn;
  }
  TapNames(const TapNames&) = delete;
  ~TapNames() { w->kn_out = nullptr; }
};

// The end of a tapped call, behind its final sync (the copies are complete): the list into the caller's buffer, the planes to the
// context — mi355tts_voc_tap_copy serves whichever call tapped last.
static int finish_taps(mi355tts_ctx* ctx, const std::shared_ptr<VocTaps>& taps, char* json, int cap) {
  const std::string s = taps->json();
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->voc_taps = taps;
  }
  return copy_json(s, json, cap, "tap list buffer too small");
}

extern "C" int mi355tts_voc_tap_copy(mi355tts_ctx* ctx, int index, float* dst, int64_t cap) {
  if (!ctx || !dst) return fail(MI355TTS_ERR_INVALID, "null argument");
  std::shared_ptr<VocTaps> taps;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    taps = ctx->voc_taps;
  }
  if (!taps || index < 0 || (size_t)index >= taps->taps.size()) return fail(MI355TTS_ERR_INVALID, "no tap %d (mi355tts_hifigan_infer_taps or mi355tts_glow_infer_taps first)", index);
  const VocTap& t = taps->taps[(size_t)index];
  const size_t n = (size_t)t.B * t.ch * t.ld;
  if ((size_t)std::max<int64_t>(cap, 0) < n) return fail(MI355TTS_ERR_TOO_SMALL, "tap %d holds %zu floats", index, n);
  HIPCHECK(hipSetDevice(ctx->device));
  if (!t.f16) {
    HIPCHECK(hipMemcpy(dst, t.dev, t.bytes, hipMemcpyDeviceToHost));
    return 0;
  }
  // octet planes [B][ch / 8][ld][8] halves -> [B][ch][ld] floats (every half is a float: exact)
  std::vector<_Float16> h(t.bytes / sizeof(_Float16));
  HIPCHECK(hipMemcpy(h.data(), t.dev, t.bytes, hipMemcpyDeviceToHost));
  const size_t noct = (size_t)t.ch / 8, ld = (size_t)t.ld;
  for (size_t b = 0; b < (size_t)t.B; ++b)
    for (size_t o = 0; o < noct; ++o)
      for (size_t col = 0; col < ld; ++col)
        for (size_t e = 0; e < 8; ++e) dst[(b * t.ch + 8 * o + e) * ld + col] = (float)h[((b * noct + o) * ld + col) * 8 + e];
  return 0;
}
