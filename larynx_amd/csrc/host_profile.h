// mi355tts host runtime — launch accounting: the launch classes and kernel names, the scope that names, counts and times a
// launch (ProfScope), the per-context sums and their three JSON renderings
// (one translation unit: included once, by host_context.h, whose context and workers derive from ProfSums and ProfLane)
#pragma once

// ------------------------------------------------------------------ the two tables
// Launch classes (mi355tts_profile_json's keys, in this order) and kernel names (mi355tts_kernel_counts_json's keys, in this
// order; the tests and bench.py's `roofline.by_kernel` index by these strings).  Each entry is written once: X(id, "string").
#define MI355TTS_KCLASSES(X) \
  X(KC_RESBLOCK, "conv_mfma.hifigan_resblock") X(KC_UPSAMPLE, "conv_mfma.hifigan_upsample") X(KC_VOC_IO, "conv_mfma.hifigan_pre_post") \
  X(KC_GLOW_ENC_CONV, "conv_mfma.glow_encoder") X(KC_GLOW_DEC_CONV, "conv_mfma.glow_decoder") X(KC_SMALL, "elementwise") \
  X(KC_MRF_NARROW, "mrf_small.hifigan_narrow_stage")
// Launches per kernel NAME are always counted (one relaxed atomic add per launch).  The class counters cannot tell a kernel from
// the fallback that would take its place (rb_group_kernel -> conv_group_kernel, rb_pair_group_kernel -> pair_group_kernel: same
// launch counts per class, same bits by design), so the device tests assert on these.
// (launch_attention's three branches: "attention_mfma_kernel" is the 256-id LDS layout, ".p768" the ATTM_MAXP layout,
// "attention_kernel" the VALU kernel)
#define MI355TTS_KNAMES(X) \
  X(KN_CONV_MFMA, "conv_mfma_kernel") X(KN_CONV_M128, "conv_mfma_kernel.m128") X(KN_CONV_GROUP, "conv_group_kernel") X(KN_RB_CONV, "rb_conv_kernel") \
  X(KN_RB_GROUP, "rb_group_kernel") X(KN_RB_GROUP_SNAKE, "rb_group_kernel.snake") X(KN_PAIR, "resblock_pair_kernel") X(KN_PAIR_GROUP, "pair_group_kernel") \
  X(KN_RB_PAIR, "rb_pair_kernel") X(KN_RB_PAIR_GROUP, "rb_pair_group_kernel") X(KN_CONV_BF16, "conv_bf16_kernel") X(KN_CONV_BF16_GROUP, "conv_bf16_group_kernel") \
  X(KN_PAIR_BF16, "pair_bf16_kernel") X(KN_PAIR_BF16_GROUP, "pair_bf16_group_kernel") X(KN_MRF_SMALL, "mrf_small_kernel") X(KN_MRF8, "mrf8_kernel") \
  X(KN_GATE16, "gate16_kernel") X(KN_GATE16_WIDE, "gate16_kernel.wide") X(KN_LIN16, "lin16_kernel") X(KN_LIN16_LN, "lin16_kernel.ln") \
  X(KN_LIN16_WIDE, "lin16_kernel.wide") X(KN_GLOW_TAIL, "glow_tail_kernel") X(KN_OPROJ_LN, "oproj_ln_kernel") X(KN_POST_CONV, "post_conv_kernel") \
  X(KN_WAVE_OUT, "wave_out_kernel") X(KN_ATTENTION, "attention_mfma_kernel") X(KN_CONV_F16, "conv_f16_kernel") X(KN_CONV_F16_GROUP, "conv_f16_group_kernel") \
  X(KN_POST_F16, "post_f16_kernel") X(KN_PACK_OCTETS, "pack_octets_kernel") X(KN_PAIR_F16_GROUP, "pair_f16_group_kernel") X(KN_WN_F16, "wn_f16_kernel") \
  X(KN_RB_GROUP_NB4, "rb_group_kernel.nb4") X(KN_GL_MAG, "griffin_lim_mag_kernel") X(KN_GL_INIT, "griffin_lim_init_kernel") X(KN_GL_ITER, "griffin_lim_iter_kernel") \
  X(KN_GL_OUT, "griffin_lim_out_kernel") X(KN_GL_INT16, "griffin_lim_int16_kernel") X(KN_GLOW_FWD, "glow_fwd_kernel") X(KN_ALIGN_SCORE, "align_score_kernel") \
  X(KN_ALIGN_PATH, "align_path_kernel") X(KN_MEL_ANALYSIS, "mel_analysis_kernel") X(KN_ATTENTION_P768, "attention_mfma_kernel.p768") X(KN_ATTENTION_VALU, "attention_kernel") \
  X(KN_LOUD_CHUNK, "loudness_chunk_kernel") X(KN_LOUD_CARRY, "loudness_carry_kernel") X(KN_LOUD_WEIGHT, "loudness_weight_kernel") \
  X(KN_LOUD_SEGMENT, "loudness_segment_kernel") X(KN_LOUD_GATE, "loudness_gate_kernel") X(KN_LOUD_APPLY, "loudness_apply_kernel") \
  X(KN_LIM_PEAK, "limiter_peak_kernel") X(KN_LIM_REDUCE, "limiter_reduce_kernel") X(KN_LIM_HOLD, "limiter_hold_kernel") \
  X(KN_LIM_CARRY, "limiter_carry_kernel") X(KN_LIM_APPLY, "limiter_apply_kernel") X(KN_PITCH, "pitch_kernel") \
  X(KN_SHIFT_MARK, "shift_mark_kernel") X(KN_SHIFT_OLA, "shift_ola_kernel")
// The first KN_PINNED names are always rendered by mi355tts_kernel_counts_json, zero or not: that key list and its order are
// ABI.  A name behind them is rendered once it has launched since the last reset, so a caller that never uses the newer entry
// points reads exactly the list it always read.
constexpr int KN_PINNED = 44;
#define MI355TTS_X_ID(id, str) id,
#define MI355TTS_X_STR(id, str) str,
enum KClass { MI355TTS_KCLASSES(MI355TTS_X_ID) KC_COUNT };
enum KName { MI355TTS_KNAMES(MI355TTS_X_ID) KN_COUNT };
static const char* const kclass_name[KC_COUNT] = {MI355TTS_KCLASSES(MI355TTS_X_STR)};
static const char* const kname_name[KN_COUNT] = {MI355TTS_KNAMES(MI355TTS_X_STR)};
#undef MI355TTS_X_ID
#undef MI355TTS_X_STR
static_assert(KC_COUNT == 7 && KN_COUNT == 58, "a new class or name goes at the END of its table (the JSON key order is ABI) and is counted here");

// ------------------------------------------------------------------ what the scope works on
struct ProfEvent {
  hipEvent_t a, b;
  int cls;
  double flop;
  int kn, sub;  // kernel name (KName, -1 = a kernel without one) and a sub-key of the launch (its output rows / channels)
};
struct ProfAcc {
  long long launches = 0;
  double ms = 0, flop = 0;
};
// The context's part: the sums of the timed launches (read and written under the context's mutex) and the name counters
struct ProfSums {
  std::atomic<bool> profiling{false};
  ProfAcc prof[KC_COUNT];
  std::map<std::pair<int, int>, ProfAcc> prof_kn[KC_COUNT];  // per class: (kernel name, sub-key) -> the same sums
  std::atomic<long long> kn[KN_COUNT] = {};                  // launches per kernel name since the last reset
};
// A worker's part: its stream, the event pairs of its timed launches until drain_profile, and the switches of its call
struct ProfLane {
  hipStream_t stream = nullptr;
  std::vector<ProfEvent> events;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> event_pool;
  // profiled FLOP of the launches that follow = the padded-batch figure x this (sum of the rows' real lengths / (B x longest))
  double flop_scale = 1.0;
  // this worker's launches are neither timed nor counted per kernel name (the dispatch self-check's own launches are not a
  // caller's: a worker-local switch, so concurrent calls on the context keep their samples and counts)
  bool quiet = false;
  // where a tapped call (mi355tts_hifigan_infer_taps / mi355tts_glow_infer_taps) learns the name its last launch was counted under; null otherwise
  int* kn_out = nullptr;
};

// ------------------------------------------------------------------ the scope
// One per launch site, around the launch: kernel() names the launch and counts it (profiling on or off: one relaxed atomic
// add, no HIP call, no allocation); with profiling on the scope also brackets the launch with an event pair, filed under the
// last name given (none: "-").  The launch helpers that have no context take their caller's scope by reference.
struct ProfScope {
  ProfSums* sums;
  ProfLane* w;
  bool on;
  ProfEvent ev;
  hipStream_t st;
  ProfScope(ProfSums* c, ProfLane* wk, int cls, double flop, hipStream_t stream = nullptr)
      : sums(c), w(wk), on(c->profiling.load() && !wk->quiet), st(stream ? stream : wk->stream) {
    if (!on) return;
    if (!w->event_pool.empty()) {
      ev.a = w->event_pool.back().first;
      ev.b = w->event_pool.back().second;
      w->event_pool.pop_back();
    } else {
      if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) {
        on = false;
        return;
      }
    }
    ev.cls = cls;
    ev.flop = flop * wk->flop_scale;
    ev.kn = -1;
    ev.sub = 0;
    hipEventRecord(ev.a, st);
  }
  ProfScope(const ProfScope&) = delete;
  // sub: the launch's output rows / channels where one name covers several shapes
  void kernel(int k, int sub = 0) {
    ev.kn = k;
    ev.sub = sub;
    if (!w->quiet) sums->kn[k].fetch_add(1, std::memory_order_relaxed);
    if (w->kn_out) *w->kn_out = k;
  }
  ~ProfScope() {
    if (!on) return;
    hipEventRecord(ev.b, st);
    w->events.push_back(ev);
  }
};

// the finished event pairs of a worker into the context's sums (`mu`: the context's mutex)
static void drain_profile(ProfSums* sums, ProfLane* w, std::mutex& mu) {
  if (w->events.empty()) return;
  std::lock_guard<std::mutex> lk(mu);
  for (auto& ev : w->events) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
      for (ProfAcc* acc : {&sums->prof[ev.cls], &sums->prof_kn[ev.cls][std::make_pair(ev.kn, ev.sub)]}) {
        acc->launches++;
        acc->ms += ms;
        acc->flop += ev.flop;
      }
    }
    w->event_pool.emplace_back(ev.a, ev.b);
  }
  w->events.clear();
}

// ------------------------------------------------------------------ behind the C ABI (mi355tts.hip holds the context's mutex
// around everything here but the name counters, which are read and written relaxed)
static void profile_reset(ProfSums& p) {
  for (auto& a : p.prof) a = ProfAcc();
  for (auto& m : p.prof_kn) m.clear();
  for (auto& k : p.kn) k.store(0, std::memory_order_relaxed);
}
// "key": {"launches": n, "ms": t, "flop": f}
static std::string acc_json(const std::string& key, const ProfAcc& a) {
  char tmp[256];
  std::snprintf(tmp, sizeof(tmp), "\"%s\": {\"launches\": %lld, \"ms\": %.6f, \"flop\": %.6e}", key.c_str(), a.launches, a.ms, a.flop);
  return tmp;
}
// {"class": {"launches": n, "ms": t, "flop": f}, ...}: every class
static std::string profile_json(const ProfSums& p) {
  std::string s = "{";
  for (int i = 0; i < KC_COUNT; ++i) s += (i ? ", " : "") + acc_json(kclass_name[i], p.prof[i]);
  return s + "}";
}
// The same sums per kernel NAME and launch sub-key (output rows of a conv launch / channels of a fused pair): {"class": {"name/sub":
// {"launches": n, "ms": t, "flop": f}, ...}, ...}, the classes with launches only; launches of kernels without a counted name are
// filed under "-".  bench.py's `roofline.by_kernel` (a driver record on an unknown box can then be compared with the builder's
// kernel by kernel).
static std::string profile_kernels_json(const ProfSums& p) {
  std::string s = "{";
  for (int i = 0; i < KC_COUNT; ++i) {
    if (p.prof_kn[i].empty()) continue;
    s += std::string(s.size() > 1 ? ", \"" : "\"") + kclass_name[i] + "\": {";
    const char* sep = "";
    for (const auto& kv : p.prof_kn[i]) {
      const int kn = kv.first.first;
      s += sep + acc_json(std::string(kn >= 0 && kn < KN_COUNT ? kname_name[kn] : "-") + "/" + std::to_string(kv.first.second), kv.second);
      sep = ", ";
    }
    s += "}";
  }
  return s + "}";
}
// {"kernel name": launches, ...} since the last reset — counted whether profiling is on or not
static std::string kernel_counts_json(const ProfSums& p) {
  std::string s = "{";
  for (int i = 0; i < KN_COUNT; ++i) {
    char tmp[128];
    const long long n = p.kn[i].load(std::memory_order_relaxed);
    if (i >= KN_PINNED && n == 0) continue;
    std::snprintf(tmp, sizeof(tmp), "%s\"%s\": %lld", i ? ", " : "", kname_name[i], n);
    s += tmp;
  }
  return s + "}";
}
// a rendering into the caller's buffer, or ERR_TOO_SMALL with `too_small` as the error text
static int copy_json(const std::string& s, char* buf, int cap, const char* too_small) {
  if ((int)s.size() + 1 > cap) return fail(MI355TTS_ERR_TOO_SMALL, "%s", too_small);
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return 0;
}

// What the two event records of a ProfScope cost by themselves: `pairs` empty pairs (hipEventRecord a, hipEventRecord b,
// nothing between) on an idle stream of `device`, median elapsed in microseconds.  A profiled launch's event time is its
// kernel's duration plus at least this (4.5 us on MI355X; rocprofv3's kernel durations do not contain it), so bench.py
// reports its event-timed launch durations with and without it.
static int profile_event_overhead(int device, int pairs, double* us_out) {
  HIPCHECK(hipSetDevice(device));
  hipStream_t st = nullptr;
  HIPCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  std::vector<float> el;
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t e = hipEventCreate(&a);
  if (e == hipSuccess) e = hipEventCreate(&b);
  for (int i = 0; i < pairs + 3 && e == hipSuccess; ++i) {
    hipEventRecord(a, st);
    hipEventRecord(b, st);
    e = hipStreamSynchronize(st);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    if (i >= 3) el.push_back(ms);  // (the first records of a new stream are slower)
  }
  if (a) hipEventDestroy(a);
  if (b) hipEventDestroy(b);
  hipStreamDestroy(st);
  if (e != hipSuccess) return fail(MI355TTS_ERR_HIP, "event overhead: %s", hipGetErrorString(e));
  std::sort(el.begin(), el.end());
  *us_out = 1000.0 * (double)el[el.size() / 2];
  return 0;
}
