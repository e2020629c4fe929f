// mi355tts host runtime — everything that selects a kernel, a tile or a schedule: the environment knobs, the context options
// (mi355tts_set_option) and the snapshot of both that one call runs under.  The only file that knows a knob's or an option's name.
// (one translation unit: included once by mi355tts.hip, ahead of host_context.h)
#pragma once

// ------------------------------------------------------------------ environment knobs
// One row per knob: field of EnvKnobs, name, type (bool = flag: set and not 0; int / long long; double), default, when it is
// read, what it does.  Defaults are the measured optimum (DESIGN.md lists the same names; tests/test_options_table.py compares).
//   PROCESS  read once, when the first context is created
//   CALL     read again whenever a call checks its worker out (snapshot_options): tests and tools move these between calls
constexpr int KNOB_UNSET = INT_MIN;  // an int knob that stands for "not in the environment" (its rule then decides)
enum KnobWhen { PROCESS, CALL };
#define MI355TTS_ENV_KNOBS(X)                                                                                                       \
  X(sync_mode, "MI355TTS_SYNC_MODE", int, 3, PROCESS, "initial g_sync_mode: 0 hipStreamSynchronize, 1 blocking event, 2 query + sleep, 3 adaptive") \
  X(queue_policy, "MI355TTS_QUEUE_POLICY", int, 0, PROCESS, "acquire_worker: 1 = an idle hardware queue first, else the BUSIEST one (probe)") \
  X(queue_probe_off, "MI355TTS_NO_QUEUE_PROBE", bool, false, PROCESS, "no measurement of which worker streams share a hardware queue") \
  X(call_coalesce_off, "MI355TTS_NO_CALL_COALESCE", bool, false, PROCESS, "every call runs alone whatever option call_coalesce says") \
  X(selfcheck_off, "MI355TTS_NO_SELFCHECK", bool, false, PROCESS, "no dispatch-order self-check (looked at again when the check would run)") \
  X(rb_tiles, "MI355TTS_RB_TILES", int, 0, PROCESS, "workgroup target per ResBlock conv launch (<= 0: 1024)")                       \
  X(glow_tiles, "MI355TTS_GLOW_TILES", int, 0, PROCESS, "workgroup target per GlowTTS conv launch (<= 0: 1024)")                    \
  X(force_tile, "MI355TTS_FORCE_TILE", int, -1, PROCESS, "pins plan_conv's tile shape (0 .. 3): sweeps")                            \
  X(ups64, "MI355TTS_UPS64", bool, true, PROCESS, "64-row upsamplers on the 64 x 64 tile; 0 = plan_conv's shape rule (A/B runs)")   \
  X(m128_off, "MI355TTS_NO_M128", bool, false, PROCESS, "no 128-row tile at all")                                                    \
  X(m128_ups_off, "MI355TTS_NO_M128_UPS", bool, false, PROCESS, "no 128-row tile for the upsamplers")                                \
  X(rb_conv_off, "MI355TTS_NO_RB_CONV", bool, false, PROCESS, "grouped 128-row launches and upsamplers on the chunked tile, as option rb_conv = 0") \
  X(group_off, "MI355TTS_NO_GROUP", bool, false, PROCESS, "no grouped launches: neither run_group nor run_pair_group")               \
  X(group_promote_off, "MI355TTS_NO_GROUP_PROMOTE", bool, false, PROCESS, "batch-1 ResBlock steps stay on the tiles plan_conv chose") \
  X(snake_off, "MI355TTS_NO_SNAKE", bool, false, PROCESS, "grouped launches keep the longest-first order")                           \
  X(pair_fusion_off, "MI355TTS_NO_PAIR_FUSION", bool, false, PROCESS, "the 32 / 64-channel stages un-fused (every mode)")            \
  X(bf16_pair_off, "MI355TTS_NO_BF16_PAIR", bool, false, PROCESS, "the 32 / 64-channel stages un-fused in the bf16 modes")           \
  X(bf_k_off, "MI355TTS_NO_BF_K", bool, false, PROCESS, "no k-split tile in the bf16 modes")                                         \
  X(bf16_ups_off, "MI355TTS_NO_BF16_UPS", bool, false, PROCESS, "upsamplers stay f32 in the bf16 modes")                             \
  X(mrf8_off, "MI355TTS_NO_MRF8", bool, false, PROCESS, "the 8-channel stage on mrf_small_kernel instead of mrf8_kernel")            \
  X(voc_out_off, "MI355TTS_NO_VOC_OUT", bool, false, PROCESS, "the generic output tail, as option voc_out = 0")                      \
  X(gate16_off, "MI355TTS_NO_GATE16", bool, false, PROCESS, "WaveNet gate convs on the 32-row tile, as option gate16 = 0")           \
  X(gate16_max_tiles, "MI355TTS_GATE16_MAX_TILES", long long, 1LL << 40, PROCESS, "gate16 only for launches of at most this many 16-row tiles") \
  X(glow_fuse_off, "MI355TTS_NO_GLOW_FUSE", bool, false, PROCESS, "no column-owner / lin16 launches, as option glow_fuse = 0")       \
  X(lin16_off, "MI355TTS_NO_LIN16", bool, false, PROCESS, "encoder convs on the generic tiles")                                      \
  X(lin16_max_tiles, "MI355TTS_LIN16_MAX_TILES", long long, 1LL << 40, PROCESS, "lin16 only for launches of at most this many tiles") \
  X(lin16_no_k1, "MI355TTS_LIN16_NO_K1", bool, false, PROCESS, "1 x 1 convs never on lin16_kernel")                                 \
  X(lin16_no_ln, "MI355TTS_LIN16_NO_LN", bool, false, PROCESS, "LayerNorm as its own launch, never lin16_kernel's prologue")        \
  X(att_big_lds, "MI355TTS_ATT_BIG_LDS", bool, false, PROCESS, "attention always on the P <= 768 instantiation (A/B runs)")         \
  X(wn_repeat, "MI355TTS_WN_REPEAT", int, 1, PROCESS, "wn_f16_kernel launched N times (probe: it is idempotent)")                   \
  X(force_tile_dynamic, "MI355TTS_FORCE_TILE_DYNAMIC", int, KNOB_UNSET, CALL, "as MI355TTS_FORCE_TILE and ahead of it (tests)")     \
  X(m128_min_tiles, "MI355TTS_M128_MIN_TILES", long long, 256, CALL, "workgroups a launch must yield before the 128-row tile is used (tests lower it)") \
  X(group_ncu, "MI355TTS_GROUP_NCU", int, KNOB_UNSET, CALL, "CUs the dispatch-order logic assumes (unset: the device's; tests)")    \
  X(promote_max_imbalance, "MI355TTS_PROMOTE_MAX_IMBALANCE", double, 1.35, CALL, "promote_group_plans: busiest CU / mean above which a step is not promoted") \
  X(rb_nb4_min_tiles, "MI355TTS_RB_NB4_MIN_TILES", int, KNOB_UNSET, CALL, "128-column ResBlock tiles from this many, whatever the load; 0 = never (unset: run_group's load rule)") \
  X(rb_pair_min_tiles, "MI355TTS_RB_PAIR_MIN_TILES", long long, 512, CALL, "tiles of the k = 11 member from which a fused step takes the 4-wave tile (tests lower it)") \
  X(bench_ablate, "MI355TTS_BENCH_ABLATE", int, 0, CALL, "mi355tts_bench_conv1d: ConvArgs::ablate (results are wrong when set)")

struct EnvKnobs {
#define X(field, name, type, def, when, doc) type field = def;
  MI355TTS_ENV_KNOBS(X)
#undef X
};
static void parse_knob(const char* e, bool* v) { *v = std::atoi(e) != 0; }
static void parse_knob(const char* e, int* v) { *v = std::atoi(e); }
static void parse_knob(const char* e, long long* v) { *v = std::atoll(e); }
static void parse_knob(const char* e, double* v) { *v = std::atof(e); }
// the rows of one read time, from the environment into `k` (a knob that is not set keeps what `k` holds: its default)
static void read_env_knobs(KnobWhen which, EnvKnobs* k) {
#define X(field, name, type, def, when, doc)                          \
  if (when == which)                                                  \
    if (const char* e = std::getenv(name)) parse_knob(e, &k->field);
  MI355TTS_ENV_KNOBS(X)
#undef X
}
// the PROCESS rows as read at the first mi355tts_create (init_process_knobs); the CALL rows stay at their defaults here
static EnvKnobs g_env;
// how a caller thread waits for its stream (mi355_sync, host_context.h): process-wide, seeded by MI355TTS_SYNC_MODE, option "sync_mode"
static std::atomic<int> g_sync_mode{3};
static void init_process_knobs() {
  static const bool once = [] {
    read_env_knobs(PROCESS, &g_env);
    g_sync_mode.store(g_env.sync_mode, std::memory_order_relaxed);
    return true;
  }();
  (void)once;
}

// ------------------------------------------------------------------ context options
#ifndef MI355TTS_CALL_COALESCE_DEFAULT
#define MI355TTS_CALL_COALESCE_DEFAULT 0  // lanes of host_join.h's whole-call coalescing (0 = off)
#endif

// Written by mi355tts_set_option while calls are in flight on other threads -> atomics.  A call reads each of them ONCE, when
// it checks its worker out (snapshot_options), so one call never mixes schedules.
struct ContextOptions {
  std::atomic<bool> serial_branches{false};   // the MRF chains fold their average into one buffer (profiling / tests)
  std::atomic<bool> adaptive_schedule{false};  // with more than one call in flight the vocoder launches the members of a grouped step one by one
  std::atomic<bool> gate16{true};     // GlowTTS WaveNet gate convs on 16-row tiles (gate16.h) when the launch is small
  std::atomic<int> gate16_wide{512};  // ... with two row tiles per workgroup in passes of at least this many 16-row tiles (0 = never; same bits)
  // GlowTTS column-owner launches (coltile.h: block tails, conv_o + LayerNorm) AND the whole-tile-in-LDS convs of
  // gate16.h's lin16_kernel (FFN / duration predictor / prenet / 1 x 1 convs, LayerNorm prologues): 0 = the generic tiles
  std::atomic<bool> glow_fuse{true};
  std::atomic<bool> voc_out{true};    // conv_post + peak and the delivery of the rows as two dedicated launches (voc_out.h); 0 = round 4's ten
  std::atomic<bool> mrf_small{true};  // narrow stages (C = 8 / 16) as one fused launch per stage (mrf_small.h)
  std::atomic<bool> mrf_group{true};  // grouped launches of the MRF chains' same-geometry convs (hifigan_forward.h)
  std::atomic<bool> rb_conv{true};    // grouped 128-row launches on the continuous-stream tile (rb_conv.h; same bits)
  std::atomic<bool> rb_pair{true};    // fused ResBlock steps (64 / 32 channels) on the 4-wave tile without a k-split (rb_pair.h)
  std::atomic<bool> rb_dil{true};     // rb_conv / rb_pair grouped launches on the kernel compiled for the step's dilation (1 / 3 / 5); 0 = the run-time-dilation kernel (same bits)
  std::atomic<bool> group_promote{true};  // batch-1 ResBlock steps move to the 128-row tile when the snake deal is balanced (promote_group_plans)
  // Grouped launches whose workgroups are all resident at once are laid out as a snake over the dispatcher's rounds
  // (group_snake_order).  That order encodes an OBSERVED dispatcher rule (workgroup i -> CU i mod #CUs);
  // mi355tts_dispatch_selfcheck times it against the plain order on this device (first 'high'-class vocoder load) and turns
  // it off where it does not win (a partitioned GPU, another CU count, a firmware that deals differently).  The ORDER of a
  // launch's workgroups never changes a result; the promotion rule (which picks the TILE, i.e. the summation order) is
  // decided from the CU count and the geometry alone and is never touched by a timing.
  std::atomic<bool> group_snake{true};
  // Whole-call coalescing (host_join.h): concurrent batch-1 mi355tts_synthesize calls become the rows of fused padded calls,
  // at most `call_coalesce` of them in flight (0 = off).  A caller that finds a lane free while other passes are in flight
  // gathers for up to `call_coalesce_window_us`; a lone caller never waits.  (Not kernel selection: read where they are used.)
  std::atomic<int> call_coalesce{MI355TTS_CALL_COALESCE_DEFAULT};
  std::atomic<int> call_coalesce_window_us{300};
};

// what mi355tts_set_option walks: `flag` options store value != 0, `count` options the value clamped at 0; the row with
// neither is the process-wide "sync_mode"
static const struct OptionRow {
  const char* name;
  std::atomic<bool> ContextOptions::*flag;
  std::atomic<int> ContextOptions::*count;
} option_table[] = {
    {"adaptive_schedule", &ContextOptions::adaptive_schedule, nullptr},
    {"mrf_small", &ContextOptions::mrf_small, nullptr},
    {"gate16", &ContextOptions::gate16, nullptr},
    {"call_coalesce", nullptr, &ContextOptions::call_coalesce},
    {"call_coalesce_window_us", nullptr, &ContextOptions::call_coalesce_window_us},
    {"glow_fuse", &ContextOptions::glow_fuse, nullptr},
    {"mrf_group", &ContextOptions::mrf_group, nullptr},
    {"rb_conv", &ContextOptions::rb_conv, nullptr},
    {"group_snake", &ContextOptions::group_snake, nullptr},
    {"group_promote", &ContextOptions::group_promote, nullptr},
    {"rb_pair", &ContextOptions::rb_pair, nullptr},
    {"rb_dil", &ContextOptions::rb_dil, nullptr},
    {"gate16_wide", nullptr, &ContextOptions::gate16_wide},
    {"voc_out", &ContextOptions::voc_out, nullptr},
    {"serial_branches", &ContextOptions::serial_branches, nullptr},
    {"sync_mode", nullptr, nullptr},
};
static int set_context_option(ContextOptions& c, const char* name, int value) {
  for (const OptionRow& r : option_table) {
    if (std::strcmp(name, r.name) != 0) continue;
    if (r.flag) {
      c.*r.flag = value != 0;
    } else if (r.count) {
      c.*r.count = value < 0 ? 0 : value;
    } else {
      if (value < 0 || value > 3) return fail(MI355TTS_ERR_INVALID, "sync_mode %d outside [0, 3]", value);
      g_sync_mode.store(value, std::memory_order_relaxed);
    }
    return 0;
  }
  return fail(MI355TTS_ERR_INVALID, "unknown option '%s'", name);
}

// ------------------------------------------------------------------ the options of ONE call
// Everything that selects a kernel, a tile or a schedule, as the call saw it when it checked its worker out: a
// mi355tts_set_option or a setenv from another thread never changes a call half way through.  Plain values, owned by the worker.
struct CallOptions {
  bool glow_fuse = true, gate16 = true, rb_conv = true, rb_pair = true, rb_dil = true, group_promote = true, group_snake = true;
  bool mrf_group = true, mrf_small = true, serial_branches = false, adaptive_schedule = false, voc_out = true;
  int gate16_wide = 512;
  int pin_tile = -1;  // mi355tts_bench_conv1d's tile shape: ahead of MI355TTS_FORCE_TILE[_DYNAMIC] (set by that entry point only)
  int ncu = 256;      // CUs as the dispatch-order logic sees them: the device's, or MI355TTS_GROUP_NCU
  EnvKnobs env;       // the PROCESS rows as g_env has them, the CALL rows as the environment had them at check-out
};
// Called by acquire_worker: EVERY entry point (the op / bench entry points and the denoiser bias too) launches under the
// context's current options and never under what the worker's previous call left behind.
static void snapshot_options(const ContextOptions& c, int device_ncu, CallOptions* o) {
  *o = CallOptions();
  o->env = g_env;
  read_env_knobs(CALL, &o->env);
  o->ncu = o->env.group_ncu != KNOB_UNSET ? o->env.group_ncu : device_ncu;
  o->glow_fuse = c.glow_fuse.load();
  o->gate16 = c.gate16.load();
  o->gate16_wide = c.gate16_wide.load();
  o->rb_conv = c.rb_conv.load();
  o->rb_pair = c.rb_pair.load();
  o->rb_dil = c.rb_dil.load();
  o->group_promote = c.group_promote.load();
  o->group_snake = c.group_snake.load();
  o->mrf_group = c.mrf_group.load();
  o->mrf_small = c.mrf_small.load();
  o->serial_branches = c.serial_branches.load();
  o->adaptive_schedule = c.adaptive_schedule.load();
  o->voc_out = c.voc_out.load();
}
