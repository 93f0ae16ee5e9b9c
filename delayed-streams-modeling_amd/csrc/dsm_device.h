// dsm_device.h — DsmDevice: the device context under both engines (dsm_engine = STT, dsm_tts = TTS), and nothing of either model.
//
// It holds what every launch helper needs — the device, its streams and fork / join events, the DSM_* knobs, device / pinned
// memory and events (handed out here, tracked here), the weight mode, the split-K workspaces, the graph slots with the capture
// state, the API lock, the profiler and the error text — and it owns all of it: teardown is the destructor and nothing
// else.  An engine derives from it and adds its model.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/dsm.h"
#include "dsm_gemm_plan.h"

#define HIPCHK_E(eng, expr)                                                                         \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess) {                                                                         \
      (eng)->set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);  \
      return DSM_ERR_DEVICE;                                                                        \
    }                                                                                               \
  } while (0)
#define HIPCHK(expr) HIPCHK_E(e, expr)

static void dsm_read_env(struct DsmDevice* e, bool stt);  // dsm_engine.hip

struct DsmDevice {
  int device = 0;
  bool opened = false;  // open() got as far as hipSetDevice: from here on there may be something to release
  // s_enc: the STT engine's encoder stream, the TTS engine's decode stream; s_model: the LM's
  hipStream_t s_enc = nullptr, s_model = nullptr;
  static constexpr int kMaxGroups = 4;
  hipStream_t s_grp[kMaxGroups] = {nullptr, nullptr, nullptr, nullptr};  // s_grp[0] is unused (group 0 runs on s_model)
  hipEvent_t ev_fork = nullptr, ev_grp_done[kMaxGroups] = {};
  bool prio_streams = false;  // streams are created with explicit priorities (the STT engine); the TTS engine's with the default
  int prio_hi = 0;
  // ---- the ten DSM_* environment variables (read by dsm_read_env, listed in include/dsm.h) and what they start from ----
  bool use_graphs = true;       // DSM_GRAPHS=0: every launch sequence stays eager (GraphSlot below)
  bool fuse_qkv = true;         // DSM_FUSE_QKV=0: keep the separate QKV reduce launch
  bool stream_prio = false;     // DSM_STREAM_PRIO=1: LM streams high, encoder stream low (STT engine)
  // DSM_FUSE_FRONT=0: the SEANet front end as three GEMM launches instead of the one fused kernel (seanet_front_kernel): the
  // test lever that the fused kernel is compared against.  (Off until r10: beside the LM's dot_mode 1 kernels the fused
  // kernel's paired init-conv chains lost a tap now and then; DESIGN.md section 8 has the cause and the fix.)
  bool fuse_front = true;
  // the GEMM plan's knobs (GemmKnobs, dsm_gemm_plan.h, which holds their defaults and what they mean)
  int chunk_loop_min_tiles = GemmKnobs().chunk_loop_min_tiles;  // DSM_CHUNK_LOOP_MIN
  int loop_depth = GemmKnobs().loop_depth;                      // DSM_LOOP_DEPTH
  int smallk_min_tiles = GemmKnobs().smallk_min_tiles;          // DSM_SMALLK_MIN
  int smallk_mt = GemmKnobs().smallk_mt;                        // DSM_SMALLK_MT
  // ---- fixed per engine and dot_mode (dsm_read_env) ----
  size_t attn_lds_pad = 60000;  // extra dynamic LDS per attention workgroup of a large launch (2 per CU; 40000 = 3 per CU)
  int dot_mode = 0;             // the engine configuration's dot_mode: 1 = the bf16-weight GEMMs in "bx3" (gemm_bx3_kernel)

  // The "open device" step of both create functions: device check, environment, the two streams.  stt: the STT engine's
  // dsm_read_env defaults and streams with explicit priorities (DSM_STREAM_PRIO=1: LM streams high, encoder stream low; off by
  // default: measured +0.5 % at B = 64 but -2.6 % at B = 400, where the encoder's share of the step is large and starving it
  // delays the next frame); the TTS engine's two streams have the default priority.
  int open(int device_id, int dot_mode_, bool stt) {
    device = device_id;
    dot_mode = dot_mode_;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) {
      set_error("no usable HIP device %d (found %d): libdsm_mi355x has no CPU fallback", device_id, ndev);
      return DSM_ERR_DEVICE;
    }
    HIPCHK_E(this, hipSetDevice(device_id));
    opened = true;
    dsm_read_env(this, stt);
    prio_streams = stt;
    int prio_lo = 0;
    if (stt && stream_prio) (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (int rc = new_stream(&s_enc, prio_lo)) return rc;
    return new_stream(&s_model, prio_hi);
  }
  int new_stream(hipStream_t* out, int prio) {
    HIPCHK_E(this, prio_streams ? hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio)
                                : hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    return 0;
  }
  // streams and "done" events of the stream groups 1 .. G - 1 (group 0 is the model stream), and the fork event
  int open_groups(int G) {
    for (int g = 1; g < G; ++g) {
      if (int rc = new_stream(&s_grp[g], prio_hi)) return rc;
      if (int rc = new_event(&ev_grp_done[g])) return rc;
    }
    return new_event(&ev_fork);
  }
  int sid(hipStream_t st) const {  // 0 = encoder, 1 = model (= group 0), 1 + g = group g
    if (st == s_enc) return 0;
    for (int g = 1; g < kMaxGroups; ++g)
      if (st == s_grp[g]) return 1 + g;
    return 1;
  }

  // ---- what the context hands out and releases: device memory, pinned host memory, events, graph slots ----
  std::mutex own_mu;  // the four lists below (two host threads may drive one engine)
  std::vector<void*> allocs, pinned;
  std::vector<hipEvent_t> events;
  template <typename T>
  int dalloc(T** out, size_t count, bool zero = true) {
    void* p = nullptr;
    size_t bytes = count * sizeof(T) + 256;  // slack: K-padding reads of the GEMM may run past a row
    HIPCHK_E(this, hipMalloc(&p, bytes));
    {
      std::lock_guard<std::mutex> lk(own_mu);
      allocs.push_back(p);
    }
    // hipMemset / hipMemcpy run on the null stream and may return before the device side is done (a pageable H2D copy
    // returns once the data is staged); the engine's streams are non-blocking, i.e. NOT ordered against the null
    // stream, so a kernel launched right after (load-time table folds, state fills) could read or be overwritten by
    // them.  Load time only: wait.
    if (zero) {
      HIPCHK_E(this, hipMemset(p, 0, bytes));
      HIPCHK_E(this, hipStreamSynchronize(nullptr));
    }
    *out = reinterpret_cast<T*>(p);
    return 0;
  }
  template <typename T>
  int upload(T** out, const T* host, size_t count) {
    if (int rc = dalloc(out, count)) return rc;
    HIPCHK_E(this, hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice));
    HIPCHK_E(this, hipStreamSynchronize(nullptr));
    return 0;
  }
  template <typename T>
  int halloc(T** out, size_t count) {  // pinned host memory, uninitialised
    void* p = nullptr;
    HIPCHK_E(this, hipHostMalloc(&p, count * sizeof(T)));
    std::lock_guard<std::mutex> lk(own_mu);
    pinned.push_back(p);
    *out = reinterpret_cast<T*>(p);
    return 0;
  }
  // hand back a dalloc / halloc before the context ends (a staging buffer that is being replaced by a larger one)
  void dfree(void* p) {
    if (!p) return;
    {
      std::lock_guard<std::mutex> lk(own_mu);
      for (size_t i = 0; i < allocs.size(); ++i)
        if (allocs[i] == p) { allocs.erase(allocs.begin() + (long)i); break; }
    }
    (void)hipFree(p);
  }
  void hfree(void* p) {
    if (!p) return;
    {
      std::lock_guard<std::mutex> lk(own_mu);
      for (size_t i = 0; i < pinned.size(); ++i)
        if (pinned[i] == p) { pinned.erase(pinned.begin() + (long)i); break; }
    }
    (void)hipHostFree(p);
  }
  int new_event(hipEvent_t* out, unsigned flags = hipEventDisableTiming) {
    HIPCHK_E(this, hipEventCreateWithFlags(out, flags));
    std::lock_guard<std::mutex> lk(own_mu);
    events.push_back(*out);
    return 0;
  }

  // ---- weight arena: every immutable weight tensor of the STT engine lives in ONE contiguous device
  // allocation, carved in load order, so that a multi-GPU launcher can fan the packed weights out with a single RCCL
  // broadcast and the other ranks attach to the received bytes without reading, converting or packing anything.
  //   W_PLAIN    no arena: upload_w == upload (the TTS engine)
  //   W_MEASURE  first pass over the checkpoint: only adds up the carve sizes
  //   W_LOAD     second pass: carve + host-to-device copy; the answers of the optional-key probes go to `manifest`
  //   W_ATTACH   carve only: the bytes are already there (received arena); probes replay `manifest`
  enum WeightMode { W_PLAIN = 0, W_MEASURE, W_LOAD, W_ATTACH };
  WeightMode wmode = W_PLAIN;
  char* arena = nullptr;
  size_t arena_size = 0, arena_off = 0;
  bool arena_owned = false;
  std::vector<uint8_t> manifest;
  size_t manifest_pos = 0;
  template <typename T>
  int upload_w(T** out, const T* host, size_t count) {
    if (wmode == W_PLAIN) return upload(out, host, count);
    const size_t bytes = (count * sizeof(T) + 256 + 255) & ~(size_t)255;  // same slack as dalloc, 256-byte aligned carves
    if (wmode != W_MEASURE) {
      if (arena_off + bytes > arena_size) {
        set_error("weight arena too small: need %zu bytes at offset %zu of %zu (config / manifest mismatch?)", bytes, arena_off, arena_size);
        return DSM_ERR_INVALID;
      }
      *out = reinterpret_cast<T*>(arena + arena_off);
      if (wmode == W_LOAD) HIPCHK_E(this, hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice));
    } else {
      *out = nullptr;
    }
    arena_off += bytes;
    return 0;
  }
  bool skip_host_weights() const { return wmode == W_MEASURE || wmode == W_ATTACH; }

  // split-K workspaces of the tiled GEMM, one per stream (0 = encoder, 1 = model); grown on first use
  static constexpr int kStreams = 1 + kMaxGroups;
  float* gemm_ws[kStreams] = {};
  size_t gemm_ws_cap[kStreams] = {};
  std::atomic<uint64_t> ws_gen{0};  // bumped whenever a workspace moves: captured graphs hold the old pointer

  // hipGraph replay of the launch-bound inner loops: the kernel sequence of one Mimi encode / decode,
  // of one LM stream group's transformer + heads, of one TTS step is captured once its shapes, pointers and first-call
  // branches have settled (two eager runs), then replayed with ONE hipGraphLaunch — ~150 kernel nodes for ~12 us of
  // host time instead of ~3.5 us each.  Every per-step variable already lives in device buffers, so the captured
  // arguments never change.  DSM_GRAPHS=0 keeps the eager path; profiling brackets force it too.
  struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    uint64_t key = 0, ws_gen = 0;
    int warm = 0;
    int failures = 0;  // captures of this sequence that did not end in a graph; after kMaxCaptureTries it stays eager
    bool disabled = false;
  };
  static constexpr int kMaxCaptureTries = 3;
  std::deque<GraphSlot> graphs;  // every slot lives here (stable addresses): the destructor finds every exec
  GraphSlot* graph_slot() {
    std::lock_guard<std::mutex> lk(own_mu);
    graphs.emplace_back();
    return &graphs.back();
  }
  // capturing: per host thread (the encoder thread may capture while the model thread launches eagerly)
  static inline thread_local bool capturing = false;
  bool capture_failed = false;
  std::atomic<uint64_t> graph_launches{0}, eager_bodies{0}, capture_failures{0};
  std::string capture_error;  // what the first failed capture reported (err_mu)
  // a capture that did not produce a graph is never silent: counted, its first reason kept for dsm_metrics
  void note_capture_failure(const char* what, hipError_t he) {
    capture_failures += 1;
    std::lock_guard<std::mutex> lk(err_mu);
    if (capture_error.empty()) {
      capture_error = what;
      if (he != hipSuccess) { capture_error += ": "; capture_error += hipGetErrorString(he); }
    }
  }
  void fill_graph_metrics(dsm_metrics* out) {
    out->graph_launches = graph_launches;
    out->eager_bodies = eager_bodies;
    out->capture_failures = capture_failures;
    std::lock_guard<std::mutex> lk(err_mu);
    snprintf(out->capture_error, sizeof out->capture_error, "%s", capture_error.c_str());
  }

  // Two host threads may drive one engine (encoder thread || model thread, srv/batched_asr.rs:314,432).  A stream capture
  // must not see the OTHER thread touch the capturing stream or an event of it: the model thread's dsm_streams_join records
  // ev_join ON the encoder stream and then makes the model stream wait for it — issued while the encoder thread is between
  // Begin and EndCapture on that stream, the record lands inside the capture and the wait pulls the model stream into it
  // (EndCapture then fails as "unjoined" / "invalidated", which is what r02 saw now and then); the same goes for
  // hipEventSynchronize / hipStreamWaitEvent on ev_done / ev_consumed against a capture on the stream of their last record.
  // A capture therefore runs alone: every entry point that issues HIP work holds api_mu shared for the whole call,
  // run_captured trades that for the exclusive side around Begin..Instantiate (a few times per engine lifetime).
  std::shared_mutex api_mu;
  static inline thread_local std::shared_lock<std::shared_mutex>* api_held = nullptr;

  // ---- per-kernel-class event timing (dsm_prof_*) ----
  unsigned prof_mask = 0;
  // one slot per stream (0 = encoder, 1 = model): the two host threads of the worker never share a slot
  int tag_gemm[kStreams] = {DSM_PROF_OTHER, DSM_PROF_OTHER, DSM_PROF_OTHER, DSM_PROF_OTHER, DSM_PROF_OTHER};
  int tag_attn[kStreams] = {DSM_PROF_OTHER, DSM_PROF_OTHER, DSM_PROF_OTHER, DSM_PROF_OTHER, DSM_PROF_OTHER};
  std::mutex prof_mu, err_mu;
  struct ProfRec {
    int tag;
    hipEvent_t a, b;
  };
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> prof_pool;
  double prof_total_us[DSM_PROF_NTAGS] = {0};
  uint64_t prof_launches[DSM_PROF_NTAGS] = {0};

  // in-kernel launch brackets (attention kernels): device buffer of (min start, max end) wall-clock pairs
  static constexpr size_t kDevTsCap = 1 << 16;
  unsigned long long* dev_ts = nullptr;
  std::vector<int> dev_ts_tags;  // tag of record i (records are handed out in launch order)
  std::vector<int> dev_ts_info;  // (stream id << 8) | kind of record i: 0 attention, 1 GEMM, 2 its reduce launch
  bool timeline = false;         // dsm_prof_timeline: GEMM launches take records too (two each: the GEMM and its reduce)
  unsigned long long* dev_ts_slot(int tag, int sid_ = 0, int kind = 0, int n = 1) {
    if (!dev_ts || !(prof_mask & (1u << tag))) return nullptr;
    std::lock_guard<std::mutex> lk(prof_mu);
    if (dev_ts_tags.size() + n > kDevTsCap) return nullptr;
    unsigned long long* p = dev_ts + 2 * dev_ts_tags.size();
    for (int i = 0; i < n; ++i) {
      dev_ts_tags.push_back(tag);
      dev_ts_info.push_back((sid_ << 8) | (kind + i));
    }
    return p;
  }

  hipEvent_t prof_event() {
    if (!prof_pool.empty()) {
      hipEvent_t ev = prof_pool.back();
      prof_pool.pop_back();
      return ev;
    }
    hipEvent_t ev = nullptr;
    (void)new_event(&ev, hipEventDefault);
    return ev;
  }
  // bracket one launch: returns an index to close with prof_end, or -1 when the class is not selected
  int prof_begin(int tag, hipStream_t st) {
    if (!(prof_mask & (1u << tag))) return -1;
    std::lock_guard<std::mutex> lk(prof_mu);
    ProfRec r{tag, prof_event(), prof_event()};
    (void)hipEventRecord(r.a, st);
    prof_recs.push_back(r);
    return (int)prof_recs.size() - 1;
  }
  void prof_end(int h, hipStream_t st) {
    if (h < 0) return;
    std::lock_guard<std::mutex> lk(prof_mu);
    (void)hipEventRecord(prof_recs[h].b, st);
  }

  std::string err;
  void set_error(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(err_mu);
    err = buf;
  }

  // Everything the context handed out goes here, in an order that is safe whatever state a failed create left behind: nothing
  // runs any more, then the graphs (they hold kernel arguments), the memory they pointed to, events, and the streams last.
  ~DsmDevice() {
    if (!opened) return;
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    for (GraphSlot& gs : graphs)
      if (gs.exec) (void)hipGraphExecDestroy(gs.exec);
    for (void* p : allocs) (void)hipFree(p);
    for (float* p : gemm_ws)
      if (p) (void)hipFree(p);
    if (arena && arena_owned) (void)hipFree(arena);
    for (void* p : pinned) (void)hipHostFree(p);
    for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
    for (hipStream_t st : s_grp)
      if (st) (void)hipStreamDestroy(st);
    if (s_enc) (void)hipStreamDestroy(s_enc);
    if (s_model) (void)hipStreamDestroy(s_model);
  }
};

// shared side of DsmDevice::api_mu for the length of one API call: EVERY entry point that issues HIP work holds it (r03;
// r02 had it on the two ticket entry points only, and the synchronous pair dsm_mimi_encode_step || dsm_asr_step_tokens of
// tests/harness ran unprotected).  Nested entry points (one public call inside another on the same thread) share the outer hold.
struct ApiShared {
  std::shared_lock<std::shared_mutex> lk;
  bool outer;
  explicit ApiShared(DsmDevice* e) : outer(DsmDevice::api_held == nullptr) {
    if (outer) {
      lk = std::shared_lock<std::shared_mutex>(e->api_mu);
      DsmDevice::api_held = &lk;
    }
  }
  ~ApiShared() { if (outer) DsmDevice::api_held = nullptr; }
};
// exclusive side, for a capture: gives up this thread's shared hold first (two threads upgrading at once would deadlock)
struct ApiExclusive {
  std::shared_lock<std::shared_mutex>* held;
  std::unique_lock<std::shared_mutex> lk;
  explicit ApiExclusive(DsmDevice* e) : held(DsmDevice::api_held) {
    if (held) held->unlock();
    lk = std::unique_lock<std::shared_mutex>(e->api_mu);
  }
  ~ApiExclusive() {
    lk.unlock();
    if (held) held->lock();
  }
};
