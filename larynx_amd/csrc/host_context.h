// mi355tts host runtime — context, per-call workers (stream + workspace + pinned staging), device-block pool
// (a call checks its worker out and gives it back through its CallFrame: host_call.h)
// (one translation unit: included once by mi355tts.hip, after the kernel headers)
#pragma once

#include "host_profile.h"

// ------------------------------------------------------------------ context
// Host wait for a stream.  hipStreamSynchronize SPINS: a caller thread burns a core for the ~4 ms its kernels run (28 ms of CPU
// per utterance with eight callers, measured), and the reference's calling pattern is a ThreadPoolExecutor of up to 32 such
// threads per process (larynx/__init__.py:66-67, :146) — times 8 ranks on a node.  Default (mode 3, adaptive): poll
// hipStreamQuery without sleeping for the first 60 us (short waits: the frame-count read-back on an idle GPU, a warm vocoder tail),
// then poll every ~20 us from nanosleep, with the calling thread's timer slack lowered to 1 us for the duration of the wait
// (the default slack of 50 us would add that much to every wake-up) and restored afterwards.
// g_sync_mode (host_options.h): 0 = hipStreamSynchronize, 1 = blocking event, 2 = query + 20 us sleep (no spin phase, default
// slack), 3 = adaptive.
static hipError_t mi355_sync(hipStream_t s) {
  const int mode = g_sync_mode.load(std::memory_order_relaxed);
  if (mode == 1) {
    // one blocking event per (thread, device): an event belongs to the device that was current when it was created
    constexpr int MAXDEV = 16;
    thread_local hipEvent_t evs[MAXDEV] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return hipStreamSynchronize(s);
    if (!evs[dev] && hipEventCreateWithFlags(&evs[dev], hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) {
      evs[dev] = nullptr;
      return hipStreamSynchronize(s);
    }
    hipError_t e = hipEventRecord(evs[dev], s);
    return e == hipSuccess ? hipEventSynchronize(evs[dev]) : e;
  }
  if (mode == 2) {
    for (;;) {
      const hipError_t e = hipStreamQuery(s);
      if (e != hipErrorNotReady) return e;
      struct timespec ts = {0, 20000};
      nanosleep(&ts, nullptr);
    }
  }
  if (mode == 3) {
    struct timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (;;) {  // spin phase
      const hipError_t e = hipStreamQuery(s);
      if (e != hipErrorNotReady) return e;
      struct timespec t1;
      clock_gettime(CLOCK_MONOTONIC, &t1);
      if ((t1.tv_sec - t0.tv_sec) * 1000000000LL + (t1.tv_nsec - t0.tv_nsec) > 60000) break;
    }
    // the calling thread's timer slack: lowered for the duration of this wait only and restored — and left alone where the
    // process may not change it (a seccomp filter that denies prctl: the sleeps then keep the default slack)
    const int slack = prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0);
    const bool lowered = slack > 1000 && prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0) == 0;
    hipError_t e;
    for (;;) {
      e = hipStreamQuery(s);
      if (e != hipErrorNotReady) break;
      struct timespec ts = {0, 20000};
      nanosleep(&ts, nullptr);
    }
    if (lowered) prctl(PR_SET_TIMERSLACK, (unsigned long)slack, 0, 0, 0);
    return e;
  }
  return hipStreamSynchronize(s);
}

struct Worker : ProfLane {  // (its stream, event pairs, flop_scale and `quiet`: host_profile.h)
  char* arena = nullptr;
  size_t arena_bytes = 0;
  size_t arena_pos = 0;
  int* pinned = nullptr;  // pinned host staging for frame counts
  size_t pinned_ints = 0;
  char* pinned_out = nullptr;  // pinned host staging for waveform outputs (grow-only)
  size_t pinned_out_bytes = 0;
  // hardware-queue group of `stream` (streams of one group run their kernels one after the other): learnt by
  // probe_queue_groups at mi355tts_reserve, -1 = not probed (a worker created on demand)
  int qgroup = -1;
  // side streams for the independent MRF branches of a HiFi-GAN stage
  hipStream_t aux[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_join[2] = {nullptr, nullptr};
  CallOptions opt;  // what selects this call's kernels, tiles and schedule: filled when the worker is checked out (acquire_worker)
};

struct mi355tts_ctx : ProfSums {  // (the profiling switch, the launch sums and the name counters: host_profile.h)
  std::shared_ptr<struct VocTaps> voc_taps;  // the last tapped call's planes (under `mu`; host_taps.h)
  int device = 0;
  int ncu = 256;  // compute units (hipGetDeviceProperties at create): the dispatch-order logic of grouped launches
  std::mutex mu;
  // every loaded model by id; `kind` is the model type's `missing` message (host_models.h; find_model / register_model: host_call.h)
  struct ModelEntry {
    const char* kind;
    std::shared_ptr<void> model;
  };
  std::map<int, ModelEntry> models;
  // window + twiddles of the Griffin-Lim kernels (griffin_lim.h), built by the first load of a Griffin-Lim or analysis model
  float* gl_table = nullptr;
  float* hann_periodic = nullptr;  // the HiFi-GAN framing's window (mel_analysis.h), built by the first analysis load
  int next_id = 1;
  std::vector<Worker*> free_workers;
  std::vector<Worker*> all_workers;
  ContextOptions opts;  // mi355tts_set_option's (host_options.h); calls read them through Worker::opt
  // calls currently holding a worker; with "adaptive_schedule" on and more than one in flight the vocoder
  // launches the members of a grouped step one by one (and never forks its MRF chains)
  std::atomic<int> active_calls{0};
  // calls in flight per hardware-queue group (index = Worker::qgroup; guarded by `mu`): acquire_worker hands out the free worker
  // whose group is the least busy
  std::vector<int> qgroup_busy;
  std::atomic<int> selfcheck_state{0};  // 0 = not run, 4 = running, 1 = snake kept, 2 = snake order disabled, 3 = skipped / failed
  float selfcheck_plain_us = 0.f, selfcheck_snake_us = 0.f;
  std::mutex join_mu;
  std::condition_variable join_cv;
  std::vector<struct CallReq*> join_q;  // waiting requests in arrival order (under join_mu, like everything below)
  int join_inflight = 0, join_rows_inflight = 0;  // fused passes in flight and the rows they carry
  bool join_gathering = false;                    // a leader-to-be is inside its gather window
  long long join_arrivals = 0;
  long long join_passes = 0, join_rows = 0;  // counters since the context was created (mi355tts_coalesce_stats)
  // recycled device blocks for the mel result objects: hipMalloc/hipFree synchronise
  // the whole device, which would serialise the concurrent per-utterance streams
  std::vector<std::pair<void*, size_t>> mel_pool;
  size_t mel_pool_cap = 256;  // raised by mi355tts_reserve to 3 x workers + slack
  std::map<void*, size_t> mel_sizes;  // true size of every block the pool has ever handed out
};

struct mi355tts_mel {
  mi355tts_ctx* ctx;
  int B, M, ld;
  float* raw = nullptr;   // [B][M][ld]
  float* voc = nullptr;   // [B][M][ld]
  int* frames_dev = nullptr;
  std::vector<int32_t> frames;
  int max_frames = 0;
  size_t raw_bytes = 0;  // allocation size of raw / voc (pool bookkeeping)
  // per-id durations [B][dur_ld] (frames each id occupies: duration_kernel's durations_out), only for a call that asked: the
  // device block the kernel wrote and its host copy, made behind the frame counts (mi355tts_mel_durations reads the latter)
  int* dur_dev = nullptr;
  int dur_ld = 0;
  std::vector<int32_t> durations;
};

static int acquire_worker(mi355tts_ctx* ctx, Worker** out) {
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->free_workers.empty()) {
      // the free worker whose hardware queue carries the fewest calls right now (ties, and workers that were never probed: the
      // most recently released one, as before)
      size_t pick = ctx->free_workers.size() - 1;
      if (!ctx->qgroup_busy.empty()) {
        // (MI355TTS_QUEUE_POLICY = 1, probe: an idle queue first, otherwise the BUSIEST one — exclusive queues for as many calls as
        // there are queues, the rest piled on one)
        const int policy = g_env.queue_policy;
        int best = 1 << 30;
        for (size_t i = ctx->free_workers.size(); i-- > 0;) {
          const int g = ctx->free_workers[i]->qgroup;
          int busy = (g >= 0 && g < (int)ctx->qgroup_busy.size()) ? ctx->qgroup_busy[g] : 0;
          if (policy == 1 && busy > 0) busy = 1000 - busy;
          if (busy < best) {
            best = busy;
            pick = i;
          }
        }
      }
      *out = ctx->free_workers[pick];
      ctx->free_workers.erase(ctx->free_workers.begin() + (long)pick);
      if ((*out)->qgroup >= 0 && (*out)->qgroup < (int)ctx->qgroup_busy.size()) ctx->qgroup_busy[(*out)->qgroup] += 1;
      (*out)->arena_pos = 0;
      (*out)->flop_scale = 1.0;
      snapshot_options(ctx->opts, ctx->ncu, &(*out)->opt);
      ctx->active_calls.fetch_add(1, std::memory_order_relaxed);
      return 0;
    }
  }
  HIPCHECK(hipSetDevice(ctx->device));
  Worker* w = new Worker();
  hipError_t e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete w;
    return fail(MI355TTS_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  w->pinned_ints = 4096;
  e = hipHostMalloc(&w->pinned, w->pinned_ints * sizeof(int), hipHostMallocDefault);
  if (e != hipSuccess) {
    hipStreamDestroy(w->stream);
    delete w;
    return fail(MI355TTS_ERR_HIP, "hipHostMalloc: %s", hipGetErrorString(e));
  }
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->all_workers.push_back(w);
  }
  ctx->active_calls.fetch_add(1, std::memory_order_relaxed);
  snapshot_options(ctx->opts, ctx->ncu, &w->opt);
  *out = w;
  return 0;
}

static void release_worker(mi355tts_ctx* ctx, Worker* w) {
  ctx->active_calls.fetch_sub(1, std::memory_order_relaxed);
  drain_profile(ctx, w, ctx->mu);
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (w->qgroup >= 0 && w->qgroup < (int)ctx->qgroup_busy.size() && ctx->qgroup_busy[w->qgroup] > 0) ctx->qgroup_busy[w->qgroup] -= 1;
  ctx->free_workers.push_back(w);
}

// grow-only workspace: a call computes its total need, then carves.
static int reserve(Worker* w, size_t bytes) {
  if (bytes <= w->arena_bytes) return 0;
  if (w->arena) {
    HIPCHECK(hipStreamSynchronize(w->stream));
    HIPCHECK(hipFree(w->arena));
    w->arena = nullptr;
    w->arena_bytes = 0;
  }
  size_t want = bytes + bytes / 8 + (1 << 20);
  hipError_t e = hipMalloc(&w->arena, want);
  if (e != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipMalloc(%zu) for workspace: %s", want, hipGetErrorString(e));
  w->arena_bytes = want;
  return 0;
}
static int reserve_pinned_out(Worker* w, size_t bytes) {
  if (bytes <= w->pinned_out_bytes) return 0;
  if (w->pinned_out) {
    HIPCHECK(hipHostFree(w->pinned_out));
    w->pinned_out = nullptr;
    w->pinned_out_bytes = 0;
  }
  const size_t want = bytes + bytes / 4 + (1 << 16);
  hipError_t e = hipHostMalloc(&w->pinned_out, want, hipHostMallocDefault);
  if (e != hipSuccess) return fail(MI355TTS_ERR_NOMEM, "hipHostMalloc(%zu) for output staging: %s", want, hipGetErrorString(e));
  w->pinned_out_bytes = want;
  return 0;
}
struct Carver {
  size_t pos = 0;
  size_t take(size_t bytes) {
    size_t off = (pos + 255) & ~(size_t)255;
    pos = off + bytes;
    return off;
  }
};
