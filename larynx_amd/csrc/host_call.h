// mi355tts host runtime — what every entry point shares around its device work: the call frame (device, worker, the drain on
// failure), the context's model table (find_model / register_model), a model's device tables (upload, pack_polyphase), the
// context's build-once device tables and the waveform intake.  The delivery of finished rows to the host (deliver_rows), the
// row types and the frame of a wave-in / wave-out call (WaveCall) follow in host_rows.h.
// (one translation unit: included once by mi355tts.hip, after host_context.h)
#pragma once

static void mel_destroy(mi355tts_mel* m);

// ------------------------------------------------------------------ the call frame
// Opened by an entry point after its argument checks: sets the device, checks a worker out, exposes ctx / w / s.  The rule it
// keeps: a worker (its arena, its staging) and a mel's pool blocks are not handed on while queued work still touches them.  A
// frame that ends without finish() waits for the worker's streams FIRST, then destroys the mel it holds, then gives the worker
// back; a finished frame waits for nothing.
struct CallFrame {
  mi355tts_ctx* ctx;
  Worker* w = nullptr;
  hipStream_t s = nullptr;
  // a mel this call made: destroyed with the frame unless take_mel() hands it to the caller
  mi355tts_mel* mel = nullptr;
  // nothing queued by this call is still running; set by wait() / finish(), or by a path that has waited for all it queued
  bool done = false;

  explicit CallFrame(mi355tts_ctx* c) : ctx(c) {}
  CallFrame(const CallFrame&) = delete;
  int open() {
    HIPCHECK(hipSetDevice(ctx->device));
    CHECK(acquire_worker(ctx, &w));
    s = w->stream;
    return 0;
  }
  hipError_t wait() {
    done = true;
    return mi355_sync(s);
  }
  int finish() {
    HIPCHECK(wait());
    HIPCHECK(hipGetLastError());
    return 0;
  }
  mi355tts_mel* take_mel() {
    mi355tts_mel* m = mel;
    mel = nullptr;
    return m;
  }
  // `n` ints of the worker's pinned staging (w->pinned)
  int pinned_ints(size_t n) const { return n <= w->pinned_ints ? 0 : fail(MI355TTS_ERR_INVALID, "batch too large"); }
  // the call's workspace and its pinned output staging, before its first queued operation (growing either frees the old block)
  int reserve(size_t arena_bytes, size_t pinned_out_bytes) {
    CHECK(::reserve(w, arena_bytes));
    return reserve_pinned_out(w, pinned_out_bytes);
  }
  ~CallFrame() {
    if (w && !done) {  // an error return behind queued work, possibly on the side streams
      mi355_sync(s);
      for (hipStream_t a : w->aux)
        if (a) mi355_sync(a);
    }
    mel_destroy(mel);
    if (!w) return;
    w->flop_scale = 1.0;
    release_worker(ctx, w);
  }
};

// ------------------------------------------------------------------ the model table
// Every call PINS its models: find_model hands out a shared_ptr copy, so mi355tts_unload only drops the context's reference
// and the id; the model is freed by whoever lets go last.  A model type names itself by its `missing` message.
template <class Model>
static int find_model(mi355tts_ctx* ctx, int id, std::shared_ptr<Model>* out) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  auto it = ctx->models.find(id);
  if (it == ctx->models.end() || it->second.kind != Model::missing) return fail(MI355TTS_ERR_NO_MODEL, Model::missing, id);
  *out = std::static_pointer_cast<Model>(it->second.model);
  return 0;
}
template <class Model>
static int register_model(mi355tts_ctx* ctx, std::shared_ptr<Model> m, int* model_out) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int id = ctx->next_id++;
  ctx->models[id] = {Model::missing, std::move(m)};
  *model_out = id;
  return 0;
}

// a model's device table: `v` into fresh device memory at `*dst` (the model's destructor frees it, also when a later step of the
// load fails); the caller has set the device
template <class T>
static int upload(T** dst, const std::vector<T>& v, const char* what) {
  if (hipMalloc(dst, v.size() * sizeof(T)) != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc %s", what);
  HIPCHECK(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// The polyphase layout of a prototype of 2 half_len + 1 taps for interpolation by `up`: table[p][t] = taps[p + t * up], rows of
// *Tp floats (*T = ceil((2 half_len + 1) / up) taps per phase, at most max_T, rounded up to 4 and zero-filled)
static int pack_polyphase(const float* taps, int half_len, int up, int max_T, int* T, int* Tp, std::vector<float>& table) {
  if (half_len < 0) return fail(MI355TTS_ERR_INVALID, "half_len %d < 0", half_len);
  const long long ntaps = 2LL * half_len + 1, per = (ntaps + up - 1) / up;
  if (per > max_T) return fail(MI355TTS_ERR_INVALID, "%lld taps per phase > %d", per, max_T);
  for (long long j = 0; j < ntaps; ++j)
    if (!std::isfinite(taps[j])) return fail(MI355TTS_ERR_INVALID, "tap %lld is not finite", j);
  *T = (int)per;
  *Tp = ((int)per + 3) & ~3;
  table.assign((size_t)up * *Tp, 0.f);
  for (long long j = 0; j < ntaps; ++j) table[(size_t)(j % up) * *Tp + (size_t)(j / up)] = taps[j];
  return 0;
}

// a device table of the context (`*slot`, guarded by ctx->mu): built and uploaded by whichever load needs it first
template <class Build>
static int context_table(mi355tts_ctx* ctx, float** slot, const char* what, Build&& build) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (*slot) return 0;
  std::vector<float> t;
  build(t);
  float* d = nullptr;
  if (hipMalloc(&d, t.size() * sizeof(float)) != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc %s", what);
  if (hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(d);
    return fail(MI355TTS_ERR_HIP, "%s upload failed", what);
  }
  *slot = d;
  return 0;
}

// ------------------------------------------------------------------ waveform intake
// The rows of a call's input waveform, f32 or int16: check() validates the sample counts, carve() takes the workspace, upload()
// sends the counts and — for a host waveform — the rows through the head of the pinned output staging (`bytes` of it) into the
// workspace at row stride Nld, tails zeroed; a device waveform is read in place.  Then d / bs / d_samples are what a kernel reads.
struct WaveIn {
  const float* f32;
  const int16_t* i16;
  const int64_t* samples;
  int B;
  int64_t ld;
  bool in_dev;
  long long Nmax = 0, total = 0;
  size_t esz = 0, Nld = 0, bytes = 0, o_n = 0, o_rows = 0;
  const void* d = nullptr;
  long long bs = 0;
  int* d_samples = nullptr;

  int check(const char* ld_name, int cap_log2) {
    for (int b = 0; b < B; ++b) {
      if (samples[b] < 0 || samples[b] > ld)
        return fail(MI355TTS_ERR_INVALID, "samples[%d]=%lld outside [0, %s=%lld]", b, (long long)samples[b], ld_name, (long long)ld);
      if (samples[b] > (1LL << cap_log2)) return fail(MI355TTS_ERR_INVALID, "samples[%d]=%lld > 2^%d", b, (long long)samples[b], cap_log2);
      Nmax = std::max(Nmax, (long long)samples[b]);
      total += samples[b];
    }
    esz = f32 ? sizeof(float) : sizeof(int16_t);
    Nld = (size_t)((Nmax + 7) & ~7LL);
    bytes = in_dev ? 0 : esz * (size_t)B * Nld;
    return 0;
  }
  void carve(Carver& cv) {
    o_n = cv.take(sizeof(int) * B);
    o_rows = cv.take(bytes);
  }
  // `counts`: B ints of w->pinned for the sample counts
  int upload(const CallFrame& f, int* counts) {
    char* base = f.w->arena;
    d_samples = (int*)(base + o_n);
    for (int b = 0; b < B; ++b) counts[b] = (int)samples[b];
    HIPCHECK(hipMemcpyAsync(d_samples, counts, sizeof(int) * B, hipMemcpyHostToDevice, f.s));
    d = f32 ? (const void*)f32 : (const void*)i16;
    bs = ld;
    if (in_dev) return 0;
    for (int b = 0; b < B; ++b) {
      char* dst = f.w->pinned_out + esz * (size_t)b * Nld;
      std::memcpy(dst, (const char*)d + esz * (size_t)b * (size_t)ld, esz * (size_t)samples[b]);
      std::memset(dst + esz * (size_t)samples[b], 0, esz * (Nld - (size_t)samples[b]));
    }
    HIPCHECK(hipMemcpyAsync(base + o_rows, f.w->pinned_out, bytes, hipMemcpyHostToDevice, f.s));
    d = base + o_rows;
    bs = (long long)Nld;
    return 0;
  }
  // the four fields every stage's kernel arguments begin with
  template <class Args>
  void bind(Args& a) const {
    a.in_f32 = f32 ? (const float*)d : nullptr;
    a.in_i16 = i16 ? (const short*)d : nullptr;
    a.in_bs = bs;
    a.samples = d_samples;
  }
};
