// dsx_api.cpp -- C ABI (include/dsx.h) of libdsx.so: parameters, contexts and
// their settings, cut lists of device blobs, generators, chunk IDs, shards.
// Every path runs through the host engine (dsx_engine.cpp).  Reference
// interfaces replaced are listed in include/dsx.h.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "dsx_engine.h"

using namespace dsx;

// the seam record is exchanged as raw bytes between ranks (and mirrored by
// desync_amd/_lib.py::Seam): its layout is part of the ABI
static_assert(sizeof(dsx_seam_t) == 7 * 8 + 4 * 4 + 8 * (DSX_SEAM_MAX_CANDS + DSX_SEAM_MAX_CUTS),
              "dsx_seam_t layout");

int set_hip_err(dsx_ctx* c, hipError_t e, const char* what) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  c->err = buf;
  return e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation ? DSX_E_NOMEM : DSX_E_HIP;
}

// --------------------------------------------------------------------------
// parameters (chunker.go:13-28, 134-171)
// --------------------------------------------------------------------------
static uint32_t discriminator_from_avg(uint64_t avg) {
  // float64, evaluated without FMA contraction (built with -ffp-contract=off)
  volatile double a = (double)avg;
  volatile double den = -1.42888852e-7 * a;
  den = den + 1.33237515;
  volatile double q = a / den;
  if (!(q >= 1.0 && q < 4294967296.0)) return 0u;
  return (uint32_t)q;
}

static uint32_t mod_inverse32(uint32_t d) {
  uint32_t x = d;
  for (int i = 0; i < 5; ++i) x *= 2u - d * x;
  return x;
}

extern "C" int dsx_abi_version(void) { return DSX_ABI_VERSION; }

extern "C" int dsx_params_init(uint64_t min, uint64_t avg, uint64_t max, dsx_params_t* out) {
  if (!out) return DSX_E_INVAL;
  if (min < 48) return DSX_E_MIN_TOO_SMALL;
  if (min > max) return DSX_E_MIN_GT_MAX;
  if (min > avg) return DSX_E_MIN_GT_AVG;
  if (avg > max) return DSX_E_AVG_GT_MAX;
  const uint32_t d = discriminator_from_avg(avg);
  if (d == 0) return DSX_E_AVG_RANGE;
  const uint32_t k = (uint32_t)__builtin_ctz(d);
  const uint32_t odd = d >> k;
  memset(out, 0, sizeof *out);
  out->min = min;
  out->avg = avg;
  out->max = max;
  out->discriminator = d;
  out->inverse_odd = mod_inverse32(odd);
  out->qbias = odd > 1u ? 1u : 0u;
  out->qmax = 0xFFFFFFFFu / d - out->qbias;
  out->rot = (int32_t)k;
  return DSX_OK;
}

extern "C" const char* dsx_strerror(int code) {
  switch (code) {
    case DSX_OK: return "ok";
    case DSX_E_MIN_TOO_SMALL: return "min chunk size too small, must be over 48";
    case DSX_E_MIN_GT_MAX: return "min chunk size must not be greater than max";
    case DSX_E_MIN_GT_AVG: return "min chunk size must not be greater than avg";
    case DSX_E_AVG_GT_MAX: return "avg chunk size must not be greater than max";
    case DSX_E_AVG_RANGE: return "avg chunk size out of range for discriminatorFromAvg";
    case DSX_E_INVAL: return "invalid argument";
    case DSX_E_CAPACITY: return "output capacity too small";
    case DSX_E_HIP: return "HIP runtime error";
    case DSX_E_NOMEM: return "out of memory";
    case DSX_E_INTERRUPTED: return "interrupted";
    case DSX_E_IO: return "I/O error";
    case DSX_E_STATE: return "invalid stream state";
    case DSX_E_INTERNAL: return "internal error";
    case DSX_E_RESYNC: return "seam records changed: all-gather them again and resolve again";
    case DSX_E_PEER: return "another rank failed (its seam record carries DSX_SEAM_ERROR)";
    default: return "unknown error";
  }
}

// --------------------------------------------------------------------------
// context
// --------------------------------------------------------------------------
static char g_create_err[256];

extern "C" int dsx_ctx_create(int device, dsx_ctx_t** out) {
  if (!out) return DSX_E_INVAL;
  *out = nullptr;
  g_create_err[0] = 0;
  dsx_ctx* c = new dsx_ctx();
  c->device = device;
#define CREATE_STEP(expr)                                                              \
  do {                                                                                 \
    const hipError_t e_ = static_cast<hipError_t>(expr);                               \
    if (e_ != hipSuccess) {                                                            \
      snprintf(g_create_err, sizeof g_create_err, "%s: %s (%d)", #expr,                \
               hipGetErrorString(e_), (int)e_);                                        \
      dsx_ctx_destroy(c);                                                              \
      return e_ == hipErrorOutOfMemory ? DSX_E_NOMEM : DSX_E_HIP;                      \
    }                                                                                  \
  } while (0)
  CREATE_STEP(hipSetDevice(device));
  hipDeviceProp_t prop;
  CREATE_STEP(hipGetDeviceProperties(&prop, device));
  c->ncu = prop.multiProcessorCount;
  // The product library reads only these DSX_* settings (INTEGRATION.md,
  // "Environment"; each has a test).  Everything measured and rejected, and
  // every diagnostic geometry, is read by libdsx_diag.so only.
  if (const char* v = getenv("DSX_TAIL_SPLIT")) c->tail_split = std::max(0, std::min(8, atoi(v)));
  if (const char* v = getenv("DSX_LANE_TARGET"))
    c->lane_target = (uint32_t)std::max(384, std::min((int)kLineLaneMax, atoi(v)));
  if (const char* v = getenv("DSX_SEG_FLOOR")) c->seg_floor = (uint64_t)std::max(0L, atol(v));
  if (const char* v = getenv("DSX_SCAN_NT")) c->scan_nt = atoi(v) & 3;
  if (const char* v = getenv("DSX_SCAN_ROTF")) c->scan_rotf = atoi(v) != 0;
  if (const char* v = getenv("DSX_DIGEST_PC")) c->digest_pc = atoi(v);
  if (const char* v = getenv("DSX_DIGEST_LPT")) c->digest_lpt = atoi(v) != 0;
  if (const char* v = getenv("DSX_INDEX_WINDOW")) c->index_window = (uint64_t)std::max(1L << 16, atol(v));
  if (const char* v = getenv("DSX_INDEX_SLOT")) c->index_slot = (uint64_t)std::max(1L << 12, atol(v));
  if (const char* v = getenv("DSX_INDEX_READERS")) c->index_readers = std::max(1, std::min(32, atoi(v)));
  if (const char* v = getenv("DSX_INDEX_HOST_TAIL")) c->index_host_tail = std::max(-1L, atol(v));
#if DSX_DIAG
  // ablation variants, alternative geometries and rejected experiments
  if (const char* m = getenv("DSX_TEST_MODE")) c->force_mode = atoi(m);
  if (const char* v = getenv("DSX_SCAN_VARIANT")) c->variant = atoi(v);
  if (const char* v = getenv("DSX_SCAN_CFG")) c->scan_cfg = std::min(5, std::max(0, atoi(v)));
  if (const char* v = getenv("DSX_DIGEST_PC_CHUNKS")) c->digest_pc_chunks = std::max(1, atoi(v));
  if (const char* v = getenv("DSX_PREFETCH")) c->prefetch_batches = std::max(0, atoi(v));
  if (const char* v = getenv("DSX_REGIONS_PER_SLOT")) c->regions_per_slot = std::max(1, atoi(v));
  if (const char* v = getenv("DSX_SCAN_LINE")) c->scan_line = atoi(v) != 0;
  if (const char* v = getenv("DSX_SCAN_TRACE")) {
    c->scan_trace = atoi(v) != 0;
    c->trace_keep = atoi(v) == 2;  // keep the traces of the last 4 pieces (slot = seq % 4)
  }
  if (const char* v = getenv("DSX_WAVE_MAJOR")) c->wave_major = atoi(v) != 0;
  if (const char* v = getenv("DSX_FIXUP_FAST")) c->fixup_fast = atoi(v) != 0;
  if (const char* v = getenv("DSX_FINISH")) c->finish = atoi(v) != 0;
  // the stitch behind the scan (tasks inside later scans)
  if (const char* v = getenv("DSX_FUSE")) c->fuse = atoi(v) != 0;
  if (const char* v = getenv("DSX_SEG_MAX")) c->seg_max_mult = std::max(1, atoi(v));
  if (const char* v = getenv("DSX_SEG_TARGET")) c->seg_target = (uint64_t)std::max(0L, atol(v));
  if (const char* v = getenv("DSX_WALK_WGS")) c->walk_wgs = std::max(1, std::min(4, atoi(v)));
  if (const char* v = getenv("DSX_WALK_NT")) c->walk_nt = atoi(v) == 576 ? 576 : 256;
  if (const char* v = getenv("DSX_DIGEST_PF")) c->digest_pf = atoi(v) != 0;
  if (const char* v = getenv("DSX_TAIL_MULT")) c->tail_mult = std::max(1, std::min(4, atoi(v)));
  if (const char* v = getenv("DSX_LANE_BYTES")) {
    const long lb = atol(v);
    if (lb >= 48 && lb % 48 == 0 && lb <= (long)kMaxLaneBytes) c->lane_bytes_override = (uint32_t)lb;
  }
  // split streams: the scan on a high-priority (or CU-masked) stream, the
  // stitch beside it on the CUs the scan leaves free
  if (const char* v = getenv("DSX_STITCH_CUS")) c->stitch_cus = std::max(0, std::min(c->ncu / 2, atoi(v)));
  if (const char* v = getenv("DSX_SCAN_MASK")) c->scan_mask = atoi(v) != 0;
#endif
  // The pipeline's streams at the highest priority: the runtime keeps
  // GPU_MAX_HW_QUEUES (4 on the box) HSA queues per priority and hands a
  // stream one at its first launch, sharing a queue once the pool is full,
  // and a kernel on a shared queue waits for the kernel ahead of it
  // (tools/queue_probe.hip, profiles/r06w, r06ai).  The default pool holds the
  // null stream and torch's streams (RCCL's among them: bench.py's N > 1
  // lanes would queue their scans behind another lane's collective); the
  // high pool holds the contexts' streams alone (copy_stream takes a queue
  // only where it is used, the file pipelines), the low pool the index
  // pipeline's digests (side_stream_create).
  {
    int least = 0, greatest = 0;
    CREATE_STEP(hipDeviceGetStreamPriorityRange(&least, &greatest));
#if DSX_DIAG
    if (const char* v = getenv("DSX_CTX_PRIO"))  // (A/B: 0 the default priority)
      if (atoi(v) == 0) greatest = 0;
#endif
    CREATE_STEP(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, greatest));
    CREATE_STEP(hipStreamCreateWithPriority(&c->copy_stream, hipStreamNonBlocking, greatest));
  }
  c->scan_stream = c->stream;
#if DSX_DIAG
  if (c->stitch_cus > 0) {
    // The scan's grid leaves stitch_cus CUs free (one per XCD at 8), and its
    // stream has the highest priority, so the dispatcher places a scan's
    // workgroups ahead of a concurrent stitch's, which fills the free CUs.
    // (A CU mask instead -- bit i is a CU of XCD i % 8 -- left one shader
    // engine per XCD a CU short of its round-robin share of the grid: a few
    // workgroups started only after the others ended, 1.9x the scan time.)
    hipStream_t ss = nullptr;
    if (c->scan_mask) {
      std::vector<uint32_t> mask((c->ncu + 31) / 32, 0u);
      for (int i = 0; i < c->ncu - c->stitch_cus; ++i) mask[i / 32] |= 1u << (i % 32);
      CREATE_STEP(hipExtStreamCreateWithCUMask(&ss, (uint32_t)mask.size(), mask.data()));
    } else {
      int least = 0, greatest = 0;
      CREATE_STEP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      const char* pv = getenv("DSX_SCAN_PRIO");
      CREATE_STEP(hipStreamCreateWithPriority(&ss, hipStreamNonBlocking,
                                              pv && atoi(pv) == 0 ? least : greatest));
    }
    c->scan_stream = ss;
    for (int i = 0; i < 2; ++i) {
      CREATE_STEP(hipEventCreateWithFlags(&c->ev_scan[i], hipEventDisableTiming));
      CREATE_STEP(hipEventCreateWithFlags(&c->ev_stitch[i], hipEventDisableTiming));
    }
  }
#endif
  // coherent, like h_ring: the tail feeder (dsx_hosttail.cpp) and dsx_progress
  // poll it while the stitch publishes into it mid-call
  CREATE_STEP(hipHostMalloc((void**)&c->h_state, sizeof(HostState), hipHostMallocCoherent));
  // coherent: dsx_result polls the seq the GPU publishes here
  CREATE_STEP(hipHostMalloc((void**)&c->h_ring, kQueueDepth * sizeof(HostState), hipHostMallocCoherent));
  memset(c->h_ring, 0, kQueueDepth * sizeof(HostState));
  c->h_cur = c->h_state;
  for (uint32_t i = 0; i < kQueueDepth; ++i)
    CREATE_STEP(hipEventCreateWithFlags(&c->q_ev[i], hipEventDisableTiming));
  CREATE_STEP(hipHostMalloc((void**)&c->h_res, 4 * sizeof(uint64_t)));
#if DSX_DIAG
  CREATE_STEP(hipHostMalloc((void**)&c->h_tasks, dsx_ctx::kTaskRing * sizeof(TaskArgs), hipHostMallocCoherent));
#endif
  memset(c->h_state, 0, sizeof(HostState));
  CREATE_STEP(c->state.ensure(c->mem, 1));
  // [0..1] overflow (piece parity); [32 + 256*parity + 32*x] the scan's work
  // queue counter x = 0..7 (one per XCD, each on its own 128-B line)
  CREATE_STEP(c->overflow.ensure(c->mem, kQueueWords));
  CREATE_STEP(hipMemset(c->overflow.p, 0, kQueueWords * sizeof(uint32_t)));
  CREATE_STEP(hipMemset(c->state.p, 0, sizeof(DevState)));
#undef CREATE_STEP
  *out = c;
  return DSX_OK;
}

extern "C" int dsx_ctx_destroy(dsx_ctx_t* c) {
  if (!c) return DSX_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  if (c->scan_stream && c->scan_stream != c->stream) (void)hipStreamSynchronize(c->scan_stream);
  if (c->h_res) (void)hipHostFree(c->h_res);
  if (c->h_tasks) (void)hipHostFree(c->h_tasks);
  index_release(c);
  stream_release(c);
  store_release(c);
  idset_release(c);
  c->mem.release_all();  // every device buffer still held, whoever's it was
  if (c->h_state) (void)hipHostFree(c->h_state);
  if (c->h_ring) (void)hipHostFree(c->h_ring);
  for (uint32_t i = 0; i < kQueueDepth; ++i)
    if (c->q_ev[i]) (void)hipEventDestroy(c->q_ev[i]);
  for (hipEvent_t e : c->pev) (void)hipEventDestroy(e);
  for (auto& v : c->q_pev)
    for (hipEvent_t e : v) (void)hipEventDestroy(e);
  for (int i = 0; i < 2; ++i) {
    if (c->ev_scan[i]) (void)hipEventDestroy(c->ev_scan[i]);
    if (c->ev_stitch[i]) (void)hipEventDestroy(c->ev_stitch[i]);
  }
  if (c->scan_stream && c->scan_stream != c->stream) (void)hipStreamDestroy(c->scan_stream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  delete c;
  return DSX_OK;
}

extern "C" const char* dsx_last_error(dsx_ctx_t* c) { return c ? c->err.c_str() : g_create_err; }

extern "C" int dsx_cancel(dsx_ctx_t* c) {
  if (!c) return DSX_E_INVAL;
  c->cancel.store(1);
  return DSX_OK;
}

// pb.Set(chunk.Start + chunk.Size) per assembled chunk (make.go:134-140): the
// end of the last confirmed chunk of the running (or last) index / cut call.
// Each piece's last stitch kernel publishes the chain position into pinned
// host memory; this reads it without touching the context's streams, so a
// second thread may call it while the call runs.  Monotone within a call.
extern "C" int dsx_progress(dsx_ctx_t* c, uint64_t* bytes) {
  if (!c || !bytes) return DSX_E_INVAL;
  uint64_t v = c->prog_done.load();
  if (c->prog_active.load()) {
    const uint64_t cur = ((volatile HostState*)c->h_state)->carry;
    if (cur > v && cur <= c->prog_len.load()) {
      uint64_t seen = v;
      while (seen < cur && !c->prog_done.compare_exchange_weak(seen, cur)) {
      }
      v = seen > cur ? seen : cur;
    }
  }
  *bytes = v;
  return DSX_OK;
}

extern "C" int dsx_debug_trace(dsx_ctx_t* c, uint64_t* out, uint64_t cap, uint64_t* n_scan,
                               uint64_t* n_walk) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !n_scan || !n_walk) return DSX_E_INVAL;
  *n_scan = c->trace_n;
  *n_walk = c->trace_walk_n;
  const uint64_t words = c->trace_keep ? 4 * (kScanTraceWords * c->trace_n + 10 * 65536ull)
                                       : kScanTraceWords * c->trace_n + 10 * c->trace_walk_n;
  if (!words || !out) return DSX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t k = std::min<uint64_t>(cap, words);
  HIPCHK(c, hipMemcpy(out, c->trace.p, k * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return DSX_OK;
}

extern "C" int dsx_copy(dsx_ctx_t* c, void* dst, const void* src, uint64_t n) {
  DSX_FLUSH_BEHIND(c);
  if (!c || (n && (!dst || !src))) return DSX_E_INVAL;
  if (!n) return DSX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(dst, src, n, hipMemcpyDefault));
  return DSX_OK;
}

// device_bytes: the total of the context's ledger (dsx_devmem.h), which every
// device allocation of the library goes through: n * sizeof(T) of each live
// DevBuf, the live stores' and ID sets' among them
// (tests/test_gpu_multiproc.py checks it against hipMemGetInfo).
extern "C" int dsx_get_stats(dsx_ctx_t* c, dsx_stats_t* out) {
  if (!c || !out) return DSX_E_INVAL;
  *out = c->stats;
  out->device_bytes = c->mem.bytes();
  return DSX_OK;
}

// In-kernel stamps of the next max_launches line-scan launches (bench.py's
// roofline: the durations of exactly the launches its timed loop runs, with
// no event between them).  Waits for the context's queued work first.
extern "C" int dsx_stamps_begin(dsx_ctx_t* c, uint64_t max_launches) {
  if (!c || max_launches == 0 || max_launches > 65536) return DSX_E_INVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->scan_stream != c->stream) HIPCHK(c, hipStreamSynchronize(c->scan_stream));
  c->stamp_slots = (uint64_t)c->ncu * (uint64_t)c->scanl_waves;  // wave slots of a line scan
  const uint64_t words = max_launches * c->stamp_slots * kStampWords;
  HIPCHK(c, grow(c, c->stamp_ring, words));
  HIPCHK(c, hipMemset(c->stamp_ring.p, 0, words * sizeof(uint64_t)));  // (end 0: slot unused)
  c->stamp_meta.clear();
  c->stamp_cap = max_launches;
  c->stamping = true;
  return DSX_OK;
}

// Stops stamping, waits for the stamped launches and reduces each one's
// per-wave records (first start, last end, summed spans) into min(cap, n)
// records in launch order; *n = the launches stamped.
extern "C" int dsx_stamps_end(dsx_ctx_t* c, dsx_scan_stamp_t* out, uint64_t cap, uint64_t* n) {
  if (!c || !n || (cap && !out)) return DSX_E_INVAL;
  const bool was = c->stamping;
  c->stamping = false;
  *n = 0;
  if (!was) return DSX_E_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->scan_stream != c->stream) HIPCHK(c, hipStreamSynchronize(c->scan_stream));
  const uint64_t k = c->stamp_meta.size();
  *n = k;
  const uint64_t m = std::min(cap, k);
  if (!m) return DSX_OK;
  const uint64_t per = c->stamp_slots * kStampWords;
  std::vector<uint64_t> raw(m * per);
  HIPCHK(c, hipMemcpy(raw.data(), c->stamp_ring.p, raw.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < m; ++i) {
    dsx_scan_stamp_t s{};
    s.seq = c->stamp_meta[i].first;
    s.bytes = c->stamp_meta[i].second;
    s.t_first = ~0ull;
    for (uint64_t w = 0; w < c->stamp_slots; ++w) {
      const uint64_t* r = &raw[i * per + w * kStampWords];
      if (r[1] == 0) continue;  // (no wave in this slot)
      s.t_first = std::min(s.t_first, r[0]);
      s.t_last = std::max(s.t_last, r[1]);
      s.wave_ticks += r[1] - r[0];
      s.wave_cycles += r[3] - r[2];
      ++s.waves;
    }
    if (!s.waves) s.t_first = 0;
    out[i] = s;
  }
  return DSX_OK;
}

// --------------------------------------------------------------------------
// cut lists of device-resident blobs (the engine: dsx_engine.cpp)
// --------------------------------------------------------------------------
// A queued cut_device call that can be stitched behind later scans: one
// line-aligned piece from 0, a candidate density the walk tasks' LDS holds.
static bool behind_ok(dsx_ctx* c, const void* d_blob, uint64_t len, const dsx_params_t* p) {
#if !DSX_DIAG
  return false;  // the stitch behind the scan is in libdsx_diag.so only
#endif
  if (!c->fuse || !c->scan_line || c->stitch_cus > 0 || c->variant) return false;
  if (len == 0 || len > kPieceMax || ((uintptr_t)d_blob & (kLine - 1)) != 0) return false;
  const uint64_t seg = stitch_seg(c, p, len);
  const double exp_per_seg = (double)seg / (double)p->discriminator + 8.0;
  return 4.0 * exp_per_seg <= (double)kTaskCand;  // wseg >= 1 with room to spare
}

// A collected call's stats: its chain state, and the scan and stitch times
// summed over its pieces' events {before scan, after scan, after gather}.
static void fill_stats(dsx_ctx* c, const HostState& s, const std::vector<hipEvent_t>& ev,
                       uint32_t npiece) {
  c->stats.chunks = s.total;
  c->stats.repaired_segments = s.repaired;
  c->stats.chunks_discarded = s.discarded;
  float scan = 0, stitch = 0;
  for (uint32_t i = 0; i < npiece; ++i) {
    float a = 0, b = 0;
    (void)hipEventElapsedTime(&a, ev[3 * i], ev[3 * i + 1]);
    (void)hipEventElapsedTime(&b, ev[3 * i + 1], ev[3 * i + 2]);
    scan += a;
    stitch += b;
  }
  c->stats.scan_ms = scan;
  c->stats.stitch_ms = stitch;
}

static int finish_call(dsx_ctx* c, uint64_t* n_out, uint64_t cap, bool* dense_retry) {
  HostState s;
  int rc = read_state(c, &s);
  if (rc) return rc;
  *dense_retry = false;
  if (s.err & kErrDense) {
    *dense_retry = true;
    return DSX_OK;
  }
  fill_stats(c, s, c->pev, c->npiece_call);
  *n_out = s.total;
  if ((s.err & kErrCapacity) || s.total > cap) return DSX_E_CAPACITY;
  return DSX_OK;
}

extern "C" int dsx_sync(dsx_ctx_t* c) {
  if (!c) return DSX_E_INVAL;
  int rc = flush_behind(c);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSX_OK;
}

extern "C" int dsx_result(dsx_ctx_t* c, uint64_t* n_out) {
  if (!c || !n_out) return DSX_E_INVAL;
  if (c->pend.empty()) return DSX_E_STATE;
  const dsx_ctx::Pending q = c->pend.front();
  c->pend.pop_front();
  HIPCHK(c, hipSetDevice(c->device));
  if (q.behind) {  // its stitch still waits for a later scan: run it now
    for (const auto& b : c->behind)
      if (b.seq == q.seq) {
        const int rc = flush_behind(c);
        if (rc) return rc;
        break;
      }
  }
  if (c->pub_host && c->pub_seq == q.seq) {  // no later scan carried its publish
    const int rc = flush_publish(c);
    if (rc) return rc;
  }
  if (q.done) HIPCHK(c, hipEventSynchronize(q.done));
  {
    // poll the published seq (published after the event when a later scan
    // or flush_publish carries it); the stream going idle without it is an error
    const volatile uint64_t* sp = &c->h_ring[q.slot].seq;
    for (uint32_t spins = 1; *sp != q.seq; ++spins) {
      if (spins % 4096u == 0) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e == hipSuccess) break;  // (seq checked below)
        if (e != hipErrorNotReady) return set_hip_err(c, e, "hipStreamQuery");
      }
      __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  HostState s;
  memcpy(&s, (const void*)&c->h_ring[q.slot], sizeof(HostState));
  if (s.seq != q.seq) {
    c->err = "stale chain state (queued call did not complete)";
    return DSX_E_INTERNAL;
  }
  if (s.err & (kErrDense | kErrRedo)) {
    // rare: redo synchronously (dense-candidate path, or the general stitch
    // with fixup_kernel's repair when a behind-the-scan stitch met a suspect
    // segment)
    if (s.err & kErrDense) c->stats.dense_fallbacks++;
    dsx_params_t p = q.p;
    return dsx_cut_device(c, q.d_blob, q.len, &p, q.out, q.cap, n_out, DSX_OUT_DEVICE);
  }
  fill_stats(c, s, c->q_pev[q.slot], q.npiece);  // (untimed queued calls record no events)
  if (q.behind) c->stats.stitch_ms = 0.0f;       // (inside later scans)
  *n_out = s.total;
  if ((s.err & kErrCapacity) || s.total > q.cap) return DSX_E_CAPACITY;
  return DSX_OK;
}

extern "C" int dsx_cut_device(dsx_ctx_t* c, const void* d_blob, uint64_t len, const dsx_params_t* p,
                              uint64_t* out_ends, uint64_t cap, uint64_t* n_out, uint32_t flags) {
  if (!c || !p || !n_out || (len && !d_blob) || (cap && !out_ends)) return DSX_E_INVAL;
  const bool dev_out = (flags & DSX_OUT_DEVICE) != 0;
  const bool queued = (flags & DSX_NO_SYNC) && dev_out;
  *n_out = 0;
  if (queued && len && c->pend.size() >= kQueueDepth) {
    c->err = "too many queued DSX_NO_SYNC calls (collect them with dsx_result)";
    return DSX_E_STATE;
  }
  // (an empty blob too: what a chain call is allowed depends on its kind alone)
  int rc = chain_begin(c, queued ? ChainKind::kCutQueued : ChainKind::kCut);
  if (rc) return rc;
  c->cancel.store(0);
  rc = ensure_attr_walk(c);
  if (rc) return rc;
  if (len == 0) return DSX_OK;  // TestChunkerEmptyFile: no chunks
  const uint64_t need = len / p->min + 2;
  const bool fuse = queued && behind_ok(c, d_blob, len, p);
  if (!fuse) {  // every other call starts after the stitches still behind
    rc = flush_tasks(c);
    if (rc) return rc;
  }
  if (!queued) {  // (a queued call's first scan publishes the previous one's state)
    rc = flush_publish(c);
    if (rc) return rc;
  }
  if (queued) {
    CallCfg cc{p, len, 0, kRound, out_ends, cap, false};
    cc.behind = fuse;
    dsx_ctx::Pending q;
    q.d_blob = d_blob;
    q.len = len;
    q.cap = cap;
    q.p = *p;
    q.out = out_ends;
    q.slot = c->q_next++ % kQueueDepth;
    q.done = c->q_ev[q.slot];
    c->h_cur = &c->h_ring[q.slot];
    // queued calls record no timing events unless DSX_TIMED: an event record
    // between two kernels of a stream costs ~6 us of GPU time (rocprofv3
    // kernel trace).  A timed call records into its slot's own events.
    const bool timed = (flags & DSX_TIMED) != 0;
    c->timing = timed;
    if (timed) std::swap(c->pev, c->q_pev[q.slot]);
    // (split streams: the next scan runs on scan_stream and waits only for
    // the stitch two pieces back, so it could publish a state the previous
    // stitch is still writing; publish_kernel then runs on the ctx stream)
    c->defer_publish = c->scan_stream == c->stream;
    rc = run_device(c, (const uint8_t*)d_blob, len, cc);
    c->defer_publish = false;
    if (timed) std::swap(c->pev, c->q_pev[q.slot]);
    q.npiece = timed ? c->npiece_call : 0u;
    c->timing = true;
    c->h_cur = c->h_state;
    if (rc) return rc;
    // an event record costs ~6 us of stream time between two jobs (rocprofv3
    // kernel trace): when finish_kernel ended the call, its last workgroup
    // publishes the state after every cut is written, and dsx_result polls it
    q.behind = fuse;
    if (fuse || (!timed && c->last_finish)) q.done = nullptr;
    else HIPCHK(c, hipEventRecord(q.done, c->stream));
    q.seq = c->piece_seq;
    c->pend.push_back(q);
    return DSX_OK;
  }
  for (int attempt = 0; attempt < 2; ++attempt) {
    CallCfg cc{p, len, 0, kRound, nullptr, 0, attempt == 1};
    if (dev_out) {
      cc.d_out = out_ends;
      cc.out_cap = cap;
    } else {
      HIPCHK(c, grow(c, c->out, need));
      cc.d_out = c->out.p;
      cc.out_cap = need;
    }
    rc = run_device(c, (const uint8_t*)d_blob, len, cc);
    if (rc) return rc;
    bool dense = false;
    rc = finish_call(c, n_out, dev_out ? cap : need, &dense);
    if (dense) {
      c->stats.dense_fallbacks++;
      continue;
    }
    if (rc) return rc;
    if (!dev_out && *n_out > cap) return DSX_E_CAPACITY;
    if (!dev_out && *n_out) {
      HIPCHK(c, hipMemcpy(out_ends, c->out.p, *n_out * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return DSX_OK;
  }
  c->err = "dense-candidate path overflowed";
  return DSX_E_INTERNAL;
}

// Many blobs packed in one device buffer -> one cut list whose chain restarts
// at every blob boundary (the engine: run_many, dsx_engine.cpp).  Every
// refusal comes before HIP is touched.
extern "C" int dsx_cut_device_many(dsx_ctx_t* c, const void* d_blob, uint64_t len,
                                   const uint64_t* blob_ends, uint64_t nblobs,
                                   const dsx_params_t* p, uint64_t* out_ends, uint64_t cap,
                                   uint64_t* n_out, uint64_t* blob_first,
                                   const dsx_many_opts_t* opts, dsx_many_totals_t* totals,
                                   uint32_t flags) {
  if (!c || !p || !n_out) return DSX_E_INVAL;
  auto refuse = [&](const char* why) {
    c->err = why;
    return DSX_E_INVAL;
  };
  if ((flags & ~DSX_OUT_DEVICE) != 0) return refuse("cut_device_many: flags other than the output's place");
  if (nblobs && !blob_ends) return refuse("cut_device_many: no blob ends");
  if (!nblobs && len) return refuse("cut_device_many: bytes but no blob");
  if (nblobs > 0xFFFFFFF0ull) return refuse("cut_device_many: more than 2^32 - 16 blobs");
  if (len && !d_blob) return refuse("cut_device_many: no buffer");
  if (cap && !out_ends) return refuse("cut_device_many: a capacity but no output");
  if (opts) {
    if (opts->reserved[0] || opts->reserved[1]) return refuse("cut_device_many: reserved option fields must be 0");
    if (opts->group_bytes > kPieceMax) return refuse("cut_device_many: more than 8 GiB per scan launch");
  }
  for (uint64_t i = 0, prev = 0; i < nblobs; prev = blob_ends[i++])
    if (blob_ends[i] < prev) return refuse("cut_device_many: blob ends decrease");
  if (nblobs && blob_ends[nblobs - 1] != len) return refuse("cut_device_many: the last blob does not end the buffer");
  if (p->min < (uint64_t)kRound || p->discriminator == 0) return refuse("cut_device_many: parameters not from dsx_params_init");

  int rc = chain_begin(c, ChainKind::kMany);
  if (rc) return rc;
  c->cancel.store(0);
  *n_out = 0;
  if (totals) *totals = dsx_many_totals_t{};
  if (nblobs == 0) return DSX_OK;
  rc = ensure_attr_walk(c);
  if (rc) return rc;
  // queued calls: as a synchronous dsx_cut_device treats them
  rc = flush_tasks(c);
  if (rc) return rc;
  rc = flush_publish(c);
  if (rc) return rc;
  const uint64_t big = opts && opts->big_blob ? opts->big_blob : many_default_big_blob(p);
  const uint64_t group = opts && opts->group_bytes ? opts->group_bytes : kPieceMax;
  return run_many(c, (const uint8_t*)d_blob, len, blob_ends, nblobs, p, out_ends, cap, n_out,
                  blob_first, big, group, totals, (flags & DSX_OUT_DEVICE) != 0);
}

// --------------------------------------------------------------------------
// synthetic data
// --------------------------------------------------------------------------
extern "C" int dsx_gen_uniform(dsx_ctx_t* c, void* d_dst, uint64_t offset, uint64_t len,
                               uint64_t seed) {
  if (!c || (len && !d_dst)) return DSX_E_INVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (!len) return DSX_OK;
  const uint64_t threads = (len + 15) / 16;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((threads + 255) / 256, 65536);
  hipLaunchKernelGGL(gen_uniform_kernel, dim3(grid), dim3(256), 0, c->stream, (uint8_t*)d_dst,
                     offset, len, seed);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSX_OK;
}

extern "C" int dsx_gen_dedup(dsx_ctx_t* c, void* d_dst, uint64_t offset, uint64_t len,
                             uint64_t seed, double p_repeat) {
  if (!c || (len && !d_dst) || !(p_repeat >= 0.0 && p_repeat < 1.0)) return DSX_E_INVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (!len) return DSX_OK;
  const uint32_t thresh = (uint32_t)std::min(4294967295.0, p_repeat * 4294967296.0);
  const uint64_t threads = (len + 15) / 16;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((threads + 255) / 256, 65536);
  hipLaunchKernelGGL(gen_dedup_kernel, dim3(grid), dim3(256), 0, c->stream, (uint8_t*)d_dst,
                     offset, len, seed, thresh);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSX_OK;
}

// --------------------------------------------------------------------------
// chunk IDs (Digest.Sum per chunk: digest.go:11-29, make.go:223)
// --------------------------------------------------------------------------
// Enqueues digest_kernel on the ctx stream.  max_n bounds the chunk count
// (the grid is sized from it; with da.range_lo the count is read on the
// device).
int launch_digest(dsx_ctx* c, DigestArgs da, uint64_t max_n, int algo, hipStream_t stream,
                  uint32_t* queue, bool serial, uint32_t max_blocks, int pc, uint64_t work) {
  // the chunks that are hashed size the grid and choose the kernel: max_n, or
  // with a take mask the number it takes
  if (!work || work > max_n) work = max_n;
  // the ctx stream, or a stream whose digests the caller runs one after
  // another (serial: dsx_index_*'s digest stream): the size-order scratch
  // (dg_order, dg_cls) is then never used by two launches at once
  const bool own = stream == nullptr || serial;
  if (!stream) stream = c->stream;
  if (!queue) {
    HIPCHK(c, c->dg_queue.ensure(c->mem, 1));
    queue = c->dg_queue.p;
  }
  // split producer/consumer kernel: one workgroup (producer + consumer wave)
  // per CU, up to digest_pc_chunks chunks per lane of the grid
  const uint64_t pc_lanes = (uint64_t)c->ncu * 64u;
  if (c->digest_pc >= 0) pc = c->digest_pc > 0 ? 1 : 0;  // (DSX_DIGEST_PC)
  if (pc > 0 || (pc < 0 && work <= pc_lanes * (uint64_t)c->digest_pc_chunks)) {
    uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((work + 63) / 64, c->ncu));
    if (max_blocks) blocks = std::min<uint64_t>(blocks, max_blocks);
    HIPCHK(c, hipMemsetAsync(queue, 0, 4, stream));
    da.queue = queue;
    da.nfirst = (uint32_t)std::min<uint64_t>(da.n, blocks * 64u);
    if (algo == DSX_DIGEST_SHA512_256)
      hipLaunchKernelGGL(digest_pc_kernel<Sha512>, dim3((uint32_t)blocks), dim3(128), 0, stream, da);
    else
      hipLaunchKernelGGL(digest_pc_kernel<Sha256>, dim3((uint32_t)blocks), dim3(128), 0, stream, da);
    HIPCHK(c, hipGetLastError());
    return DSX_OK;
  }
  // Lanes: exactly the workgroups that are resident at once (occupancy is set
  // by VGPRs: 2 per CU for SHA-512, 3 without the prefetch, 4 for SHA-256),
  // every lane pulling chunks
  // from the queue.  A larger grid would hand its non-resident workgroups a
  // static share that starts only when the first wave of workgroups is done.
  int per_cu = 0;
  const bool sha512 = algo == DSX_DIGEST_SHA512_256;
#if DSX_DIAG
  const bool pf = c->digest_pf != 0;
#else
  constexpr bool pf = true;
#endif
  const void* kern = sha512 ? (const void*)digest_kernel<Sha512, true>
                            : (const void*)digest_kernel<Sha256, true>;
#if DSX_DIAG
  if (!pf)
    kern = sha512 ? (const void*)digest_kernel<Sha512, false>
                  : (const void*)digest_kernel<Sha256, false>;
#endif
  HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kDigestThreads, 0));
  if (per_cu < 1) per_cu = 1;
  uint64_t blocks = std::max<uint64_t>(
      1, std::min<uint64_t>((work + kDigestThreads - 1) / kDigestThreads,
                            (uint64_t)per_cu * (uint64_t)c->ncu));
  if (max_blocks) blocks = std::min<uint64_t>(blocks, max_blocks);
  HIPCHK(c, hipMemsetAsync(queue, 0, 4, stream));
  da.queue = queue;
  da.nfirst = (uint32_t)std::min<uint64_t>(da.n, blocks * kDigestThreads);
  // the chunks go out longest first (a counting sort by size class, three
  // small passes on the same stream): with more chunks than lanes the long
  // chains start in the first round; with fewer, each wave's 64 static chunks
  // are of one size, so no lane idles behind a longer neighbour
  if (own && c->digest_lpt && max_n >= 8u * kDigestThreads && max_n < (1ull << 32)) {
    HIPCHK(c, grow(c, c->dg_order, max_n));
    HIPCHK(c, c->dg_cls.ensure(c->mem, 2 * kSizeClasses));
    HIPCHK(c, hipMemsetAsync(c->dg_cls.p, 0, kSizeClasses * sizeof(uint32_t), stream));
    // (a take mask: the order lists the chunks taken and ends at the first 0xFFFFFFFF)
    if (da.take) HIPCHK(c, hipMemsetAsync(c->dg_order.p, 0xFF, max_n * sizeof(uint32_t), stream));
    const dim3 tiles((uint32_t)((max_n + kOrderTile - 1) / kOrderTile));
    hipLaunchKernelGGL(digest_order_count_kernel, tiles, dim3(256), 0, stream, da, c->dg_cls.p);
    hipLaunchKernelGGL(digest_order_scan_kernel, dim3(1), dim3(kSizeClasses), 0, stream,
                       (const uint32_t*)c->dg_cls.p, c->dg_cls.p + kSizeClasses);
    hipLaunchKernelGGL(digest_order_scatter_kernel, tiles, dim3(256), 0, stream, da,
                       c->dg_cls.p + kSizeClasses, c->dg_order.p);
    HIPCHK(c, hipGetLastError());
    da.order = c->dg_order.p;
  }
  if (sha512 && pf)
    hipLaunchKernelGGL((digest_kernel<Sha512, true>), dim3((uint32_t)blocks), dim3(kDigestThreads),
                       0, stream, da);
  else if (pf)
    hipLaunchKernelGGL((digest_kernel<Sha256, true>), dim3((uint32_t)blocks), dim3(kDigestThreads),
                       0, stream, da);
#if DSX_DIAG
  else if (sha512)
    hipLaunchKernelGGL((digest_kernel<Sha512, false>), dim3((uint32_t)blocks), dim3(kDigestThreads),
                       0, stream, da);
  else
    hipLaunchKernelGGL((digest_kernel<Sha256, false>), dim3((uint32_t)blocks), dim3(kDigestThreads),
                       0, stream, da);
#endif
  HIPCHK(c, hipGetLastError());
  return DSX_OK;
}

extern "C" int dsx_chunk_ids(dsx_ctx_t* c, const void* d_blob, uint64_t len, uint64_t start,
                             const uint64_t* ends, uint64_t n, void* ids, uint32_t flags,
                             int algo) {
  DSX_FLUSH_BEHIND(c);
  if (!c || (n && (!d_blob || !ends || !ids)) || (algo != DSX_DIGEST_SHA512_256 &&
                                                   algo != DSX_DIGEST_SHA256))
    return DSX_E_INVAL;
  if ((flags & ~(DSX_OUT_DEVICE | DSX_ENDS_DEVICE)) != 0) return DSX_E_INVAL;
  if (n == 0) return DSX_OK;
  if (n > 0xFFFFFFF0ull) return DSX_E_INVAL;
  if (!(flags & DSX_ENDS_DEVICE)) {
    // chunks must lie inside the blob, in order (a hand-built index could
    // otherwise send the kernel past the end of the buffer); device-resident
    // ends are bounds-checked per chunk by the kernel instead, which skips a
    // chunk outside the blob and hashes every other one
    uint64_t prev = start;
    for (uint64_t i = 0; i < n; ++i) {
      if (ends[i] < prev || ends[i] > len) {
        c->err = "chunk ends must be non-decreasing, start <= ends[0], ends[n-1] <= len";
        return DSX_E_INVAL;
      }
      prev = ends[i];
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  const uint64_t* d_ends = ends;
  if (!(flags & DSX_ENDS_DEVICE)) {
    HIPCHK(c, grow(c, c->dg_ends, n));
    HIPCHK(c, hipMemcpyAsync(c->dg_ends.p, ends, n * 8, hipMemcpyHostToDevice, c->stream));
    d_ends = c->dg_ends.p;
  }
  uint8_t* d_ids = (uint8_t*)ids;
  if (!(flags & DSX_OUT_DEVICE)) {
    HIPCHK(c, grow(c, c->dg_ids, n * 32));
    d_ids = c->dg_ids.p;
  }
  DigestArgs da{};
  da.blob = (const uint8_t*)d_blob;
  da.len = len;
  da.ends = d_ends;
  da.first_start = start;
  da.n = n;
  da.ids = d_ids;
  int rc = launch_digest(c, da, n, algo);
  if (rc) return rc;
  if (!(flags & DSX_OUT_DEVICE))
    HIPCHK(c, hipMemcpyAsync(ids, d_ids, n * 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSX_OK;
}

// --------------------------------------------------------------------------
// diagnostics: GPU boundary predicate vs h % d == d-1
// --------------------------------------------------------------------------
extern "C" int dsx_selftest_boundary(dsx_ctx_t* c, const dsx_params_t* p, int mode, uint64_t h0,
                                     uint64_t n, uint64_t* mismatches) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !p || !mismatches) return DSX_E_INVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (mode < 0) mode = pick_mode(c, p->discriminator);
  const uint32_t d = p->discriminator;
  if (mode > 2 || (mode == 2 && (d & (d - 1u)) == 0)) return DSX_E_INVAL;  // MODE 2 needs dodd > 1
  DevBuf<unsigned long long> m;
  HIPCHK(c, m.ensure(c->mem, 1));  // (an early return leaves it to the ledger)
  HIPCHK(c, hipMemsetAsync(m.p, 0, 8, c->stream));
  hipLaunchKernelGGL(boundary_selftest_kernel, dim3(4096), dim3(256), 0, c->stream, make_tc(p),
                     mode, h0, n, m.p);
  HIPCHK(c, hipGetLastError());
  unsigned long long v = 0;
  HIPCHK(c, hipMemcpyAsync(&v, m.p, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  m.release();
  *mismatches = v;
  return DSX_OK;
}

// --------------------------------------------------------------------------
// multi-GPU shards (split-and-align across ranks, make.go:22-163 / 277-327)
// --------------------------------------------------------------------------
// Chunks the shard from the cut `entry` (shard_start: speculative, make.go's
// worker at span*i; or the true entry cut on a re-walk), builds the seam
// record in c->d_seam, leaves the shard's cuts in c->out and waits.
// The first run scans the bytes and keeps every piece's candidate lists; a
// re-walk (rewalk = true) only re-runs the stitch over the kept lists from
// the new entry: O(candidates), no byte is read again.  (Pieces that needed
// the dense-candidate path keep no lists; their re-walk scans again.)
// With async, nothing waits: the chain state is not read back (a stitch
// error, including the overflow that the synchronous path retries on the
// dense path, is published as DSX_SEAM_REDO in the record, see
// seam_finalize_kernel) and sh.nspec stays unknown (the emit kernel reads the
// count on the device).
static int shard_run(dsx_ctx* c, uint64_t entry, uint32_t rec_flags, bool rewalk,
                     bool async = false) {
  auto& sh = c->sh;
  const dsx_params_t* p = &sh.p;
  const bool is_last = sh.start + sh.len == sh.total;
  const uint64_t need = sh.len / p->min + 4;
  const uint64_t wend0 = sh.start + std::min<uint64_t>(sh.len, 32 * p->max);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, grow(c, c->d_seam, 1));
  const bool stitch_only = rewalk && !sh.dense && sh.nkept > 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (c->cancel.load()) return DSX_E_INTERRUPTED;
    HIPCHK(c, grow(c, c->out, need));
    const bool dense = attempt == 1 || (rewalk && sh.dense);
    CallCfg cc{p, sh.total, entry, kRound, c->out.p, need, dense};
    cc.halo0 = sh.start > 0 ? sh.halo : 0;
    int rc = DSX_OK;
    if (stitch_only) {
      HIPCHK(c, c->zero_word.ensure(c->mem, 1));
      HIPCHK(c, hipMemsetAsync(c->zero_word.p, 0, 4, c->stream));
      hipLaunchKernelGGL(state_init_kernel, dim3(1), dim3(64), 0, c->stream, (DevState*)c->state.p,
                         entry);
      HIPCHK(c, hipGetLastError());
      c->npiece_call = 0;
      for (size_t i = 0; i < sh.nkept && !rc; ++i) {
        PieceCands pc = sh.kept[i].pc;
        pc.overflow = c->zero_word.p;  // (the scan succeeded: no overflow)
        rc = launch_stitch(c, cc, pc, sh.kept[i].P, sh.kept[i].len,
                           is_last && i + 1 == sh.nkept, ++c->piece_seq, false);
      }
      if (rc) return rc;
      // (no seam_cands_kernel: a re-walked record carries no window,
      // seam_finalize_kernel empties its lists)
    } else {
      sh.nkept = 0;  // (the buffers are reused)
      cc.keep = dense ? nullptr : &sh.kept;
      sh.dense = dense;
      rc = reset_state(c, entry);
      if (rc) return rc;
      const uint64_t piece = cc.dense ? kDensePiece : kPieceMax;
      for (uint64_t off = 0; off < sh.len; off += piece) {
        const uint64_t n = std::min(piece, sh.len - off);
        PieceCands pc{};
        rc = enqueue_piece(c, cc, sh.d + off, off + cc.halo0, sh.start + off, n,
                           is_last && off + n == sh.len, &pc);
        if (rc) return rc;
        if (off == 0) {
          // the window candidates come from the first piece's region lists
          pc.overflow = nullptr;
          hipLaunchKernelGGL(seam_cands_kernel, dim3(1), dim3(64), 0, c->stream, pc, sh.start,
                             wend0, c->d_seam.p);
          HIPCHK(c, hipGetLastError());
        }
      }
    }
    hipLaunchKernelGGL(seam_finalize_kernel, dim3(1), dim3(1), 0, c->stream, c->d_seam.p,
                       (const uint64_t*)c->out.p, (const DevState*)c->state.p, sh.start, sh.len,
                       sh.total, wend0, entry, (is_last ? (uint32_t)DSX_SEAM_LAST : 0u) | rec_flags);
    HIPCHK(c, hipGetLastError());
    if (async) {
      sh.nspec = ~0ull;
      return DSX_OK;
    }
    HostState st;
    rc = read_state(c, &st);
    if (rc) return rc;
    if ((st.err & kErrDense) && !stitch_only) {
      c->stats.dense_fallbacks++;
      continue;
    }
    if (st.err) {
      c->err = "shard: stitch error";
      return DSX_E_INTERNAL;
    }
    sh.nspec = st.total;
    c->stats.chunks = st.total;
    return DSX_OK;
  }
  c->err = "dense-candidate path overflowed";
  return DSX_E_INTERNAL;
}

// Copies the ctx's seam record to the caller's (host or device) record; a
// device record is left in flight on the ctx stream when `wait` is false.
static int seam_out(dsx_ctx* c, dsx_seam_t* seam, bool dev, bool wait = true) {
  HIPCHK(c, hipMemcpyAsync(seam, c->d_seam.p, sizeof(dsx_seam_t),
                           dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  if (wait || !dev) HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSX_OK;
}

extern "C" int dsx_shard_local(dsx_ctx_t* c, const void* d_shard, uint64_t halo,
                               uint64_t shard_start, uint64_t shard_len, uint64_t total,
                               const dsx_params_t* p, dsx_seam_t* seam, uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !p || !seam || (shard_len && !d_shard) || shard_start + shard_len > total ||
      (flags & ~(DSX_SEAM_DEVICE | DSX_NO_SYNC)) != 0 ||
      ((flags & DSX_NO_SYNC) && !(flags & DSX_SEAM_DEVICE)))
    return DSX_E_INVAL;
  const bool async = (flags & DSX_NO_SYNC) != 0;
  if (shard_start > 0 && halo < kRound) return DSX_E_INVAL;
  // (the shard of an earlier dsx_shard_local is gone from here on; this
  // call's own run below, and shard_outcome's re-walk and redo, own the new one)
  int rc = chain_begin(c, ChainKind::kShardLocal);
  if (rc) return rc;
  c->cancel.store(0);
  rc = ensure_attr_walk(c);
  if (rc) return rc;
  auto& sh = c->sh;
  sh.d = (const uint8_t*)d_shard;
  sh.halo = halo;
  sh.start = shard_start;
  sh.len = shard_len;
  sh.total = total;
  sh.p = *p;
  sh.nspec = 0;
  if (shard_len == 0) {
    dsx_seam_t z;
    memset(&z, 0, sizeof z);
    z.shard_start = z.exit_cut = z.window_end = z.entry = shard_start;
    z.total = total;
    z.first_cand_beyond = UINT64_MAX;
    z.flags = shard_start == total ? DSX_SEAM_LAST : 0u;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, grow(c, c->d_seam, 1));
    HIPCHK(c, hipMemcpyAsync(c->d_seam.p, &z, sizeof z, hipMemcpyHostToDevice, c->stream));
    // no chain runs: without this shard_emit_kernel would count the cuts of
    // the context's previous call (st->total) as this shard's speculative ones
    hipLaunchKernelGGL(state_init_kernel, dim3(1), dim3(64), 0, c->stream, (DevState*)c->state.p,
                       shard_start);
    HIPCHK(c, hipGetLastError());
    c->owner.shard_ready();
    return seam_out(c, seam, (flags & DSX_SEAM_DEVICE) != 0);
  }
  rc = shard_run(c, shard_start, 0u, false, async);
  if (rc) return rc;
  c->owner.shard_ready();
  return seam_out(c, seam, (flags & DSX_SEAM_DEVICE) != 0, !async);
}

// The resolve outcome published by shard_emit_kernel (h_res), interpreted on
// the host: DSX_OK with the count, DSX_E_PEER, or DSX_E_RESYNC after this
// rank re-walked (a seam that did not converge) or redid (DSX_SEAM_REDO) its
// shard and rewrote `my_seam`.  A failed re-walk / redo marks `my_seam`
// DSX_SEAM_ERROR and returns its error.
static int shard_outcome(dsx_ctx* c, int rank, dsx_seam_t* my_seam, bool seam_dev, uint64_t cap,
                         uint64_t* n_out) {
  const uint64_t status = c->h_res[0], n = c->h_res[1], entry = c->h_res[2];
  *n_out = 0;
  if (status == ~0ull) {
    c->err = "shard: resolve did not publish its result";
    return DSX_E_INTERNAL;
  }
  if (status == kSeamPeerFailed) return DSX_E_PEER;
  if (status != 0) {
    // kSeamRedo: rank `entry` redoes its shard from its own start; otherwise
    // seam `status - 1` did not converge inside its window and its owner
    // re-walks its shard from the true entry cut; either way the owner
    // republishes its record
    const bool redo = status == kSeamRedo;
    const int failing = redo ? (int)entry : (int)(status - 1);
    if (failing == rank) {
      auto& sh = c->sh;
      int rc = redo ? shard_run(c, sh.start, 0u, false) : shard_run(c, entry, DSX_SEAM_REWALKED, true);
      if (rc) {
        // publish the failure in this rank's record: the peers' next resolve
        // returns DSX_E_PEER (no rank waits for a record forever)
        const size_t off = offsetof(dsx_seam_t, flags);
        uint32_t fl = 0;
        const hipMemcpyKind d2h = seam_dev ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
        const hipMemcpyKind h2d = seam_dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost;
        (void)hipStreamSynchronize(c->stream);
        if (hipMemcpy(&fl, (const uint8_t*)my_seam + off, 4, d2h) == hipSuccess) {
          fl |= DSX_SEAM_ERROR;
          (void)hipMemcpy((uint8_t*)my_seam + off, &fl, 4, h2d);
        }
        return rc;
      }
      if (redo)
        c->stats.dense_fallbacks++;
      else
        c->stats.repaired_segments++;
      rc = seam_out(c, my_seam, seam_dev);
      if (rc) return rc;
    }
    return DSX_E_RESYNC;
  }
  *n_out = n;
  if (n > cap) return DSX_E_CAPACITY;
  return DSX_OK;
}

extern "C" int dsx_shard_resolve(dsx_ctx_t* c, const dsx_seam_t* all, int nranks, int rank,
                                 dsx_seam_t* my_seam, uint64_t* out_ends, uint64_t cap,
                                 uint64_t* n_out, uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !all || nranks < 1 || rank < 0 || rank >= nranks || !n_out || !my_seam ||
      (cap && !out_ends) || (flags & ~(DSX_SEAM_DEVICE | DSX_OUT_DEVICE)) != 0)
    return DSX_E_INVAL;
  auto& sh = c->sh;
  // a chain call since dsx_shard_local left another call's cuts in c->out and
  // c->state: a stale shard never resolves to a list
  if (int rc = c->owner.resolve(&c->err)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const bool seam_dev = (flags & DSX_SEAM_DEVICE) != 0, out_dev = (flags & DSX_OUT_DEVICE) != 0;
  const dsx_seam_t* d_all = all;
  if (!seam_dev) {
    HIPCHK(c, grow(c, c->d_all, (size_t)nranks));
    HIPCHK(c, hipMemcpyAsync(c->d_all.p, all, sizeof(dsx_seam_t) * nranks, hipMemcpyHostToDevice,
                             c->stream));
    d_all = c->d_all.p;
  }
  HIPCHK(c, grow(c, c->d_ext, DSX_SEAM_MAX_CUTS + 4));
  HIPCHK(c, grow(c, c->d_info, 8));
  hipLaunchKernelGGL(seam_resolve_kernel, dim3(1), dim3(64), 0, c->stream, d_all, nranks, rank,
                     sh.p.min, sh.p.max, c->d_ext.p, c->d_info.p);
  HIPCHK(c, hipGetLastError());
  const uint64_t most = (sh.nspec == ~0ull ? sh.len / sh.p.min + 4 : sh.nspec) + DSX_SEAM_MAX_CUTS;
  uint64_t* dst = out_ends;
  uint64_t dcap = cap;
  if (!out_dev) {
    HIPCHK(c, grow(c, c->d_emit, most));
    dst = c->d_emit.p;
    dcap = most;
  }
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((most + 255) / 256, 4096);
  c->h_res[0] = ~0ull;
  hipLaunchKernelGGL(shard_emit_kernel, dim3(blocks), dim3(256), 0, c->stream,
                     (const uint64_t*)c->d_info.p, (const uint64_t*)c->d_ext.p,
                     (const uint64_t*)c->out.p, (const DevState*)c->state.p, dst, dcap,
                     (volatile uint64_t*)c->h_res, (int32_t*)nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc = shard_outcome(c, rank, my_seam, seam_dev, cap, n_out);
  if (rc) return rc;
  const uint64_t n = *n_out;
  if (!out_dev && n)
    HIPCHK(c, hipMemcpy(out_ends, c->d_emit.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return DSX_OK;
}

extern "C" int dsx_shard_resolve_async(dsx_ctx_t* c, const dsx_seam_t* all, int nranks, int rank,
                                       uint64_t* out_ends, uint64_t cap, int32_t* d_code) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !all || nranks < 1 || rank < 0 || rank >= nranks || !out_ends || !d_code)
    return DSX_E_INVAL;
  auto& sh = c->sh;
  // a chain call since dsx_shard_local left another call's cuts in c->out and
  // c->state: a stale shard never resolves to a list
  if (int rc = c->owner.resolve(&c->err)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, grow(c, c->d_ext, DSX_SEAM_MAX_CUTS + 4));
  HIPCHK(c, grow(c, c->d_info, 8));
  hipLaunchKernelGGL(seam_resolve_kernel, dim3(1), dim3(64), 0, c->stream, all, nranks, rank,
                     sh.p.min, sh.p.max, c->d_ext.p, c->d_info.p);
  HIPCHK(c, hipGetLastError());
  const uint64_t most = sh.len / sh.p.min + 4 + DSX_SEAM_MAX_CUTS;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((std::min(most, cap) + 255) / 256 + 1, 4096);
  c->h_res[0] = ~0ull;
  hipLaunchKernelGGL(shard_emit_kernel, dim3(blocks), dim3(256), 0, c->stream,
                     (const uint64_t*)c->d_info.p, (const uint64_t*)c->d_ext.p,
                     (const uint64_t*)c->out.p, (const DevState*)c->state.p, out_ends, cap,
                     (volatile uint64_t*)c->h_res, d_code);
  HIPCHK(c, hipGetLastError());
  sh.pend_rank = rank;
  sh.pend_cap = cap;
  c->owner.resolve_launched();
  return DSX_OK;
}

extern "C" int dsx_shard_collect(dsx_ctx_t* c, dsx_seam_t* my_seam, const int32_t* d_agreed,
                                 int32_t* agreed, uint64_t* n_out) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !my_seam || !n_out || (d_agreed && !agreed)) return DSX_E_INVAL;
  auto& sh = c->sh;
  if (int rc = c->owner.collect(&c->err)) {
    // (a stale shard's emit may still be writing the caller's list)
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  int32_t* h_code = (int32_t*)(c->h_res + 3);
  if (d_agreed)
    HIPCHK(c, hipMemcpyAsync(h_code, d_agreed, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the step's one host wait
  if (d_agreed) *agreed = *h_code;
  if (d_agreed && *h_code >= 2) {
    // a rank failed this round: report this rank's own failure if it has one
    const uint64_t status = c->h_res[0], n = c->h_res[1];
    *n_out = 0;
    if (status == ~0ull) return DSX_E_INTERNAL;
    if (status == 0 && n > sh.pend_cap) {
      *n_out = n;
      return DSX_E_CAPACITY;
    }
    return DSX_E_PEER;
  }
  int rc = shard_outcome(c, sh.pend_rank, my_seam, true, sh.pend_cap, n_out);
  if (rc == DSX_OK) c->stats.chunks = *n_out;
  return rc;
}

extern "C" int dsx_ctx_stream(dsx_ctx_t* c, void** stream) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !stream) return DSX_E_INVAL;
  *stream = (void*)c->stream;
  return DSX_OK;
}
