// dsx_index.cpp -- IndexFromFile on the GPU: bytes from a file descriptor or
// host memory -> cut list + chunk IDs (include/dsx.h: dsx_index_fd,
// dsx_index_host).
//
// Reference: IndexFromFile (make.go:22-163) chunks the file with n goroutines
// (split-and-align) and computes Digest.Sum of every chunk (make.go:223,
// digest.go:11-29); GetFileSize (ioctl_linux.go:63-84) sizes regular files
// and block devices.
//
// Pipeline (one context, reader threads, HIP streams in three priority pools
// so that none shares an HSA queue with another -- tools/queue_probe.hip):
//   reader threads  pread/memcpy 32 MiB pieces into a ring of pinned slots
//                   (the file's last 32 MiB in 8 MiB pieces);
//   copy_stream     H2D of each piece into the current HBM window (high);
//   stream          scan + stitch (dsx_scan.hip, dsx_stitch.hip) every
//                   32 MiB, the chain state carried on the device; at the
//                   end of a window a snapshot of {total cuts, carried cut}
//                   (high);
//   idx_side[0..3]  the windows' digests (idx_side[0] = idx_dg_stream) and,
//                   in a one-window call, the GPU's shares of the window
//                   during the read (low);
//   tail feeder     the last window's long chunks hashed on the host as the
//                   stitches confirm them (its copy stream at the default
//                   priority), the GPU's last digest skipping them.
// Two windows alternate, so the digest of window w overlaps the H2D and scan
// of window w+1.  A window starts with the last max + 128 bytes of the
// previous one: the carried cut lies in (P - max, P] (dsx_stitch.hip), so the
// unfinished chunk and the scan's 48-byte warm-up are always in HBM.  No host
// round trip happens until the end of the file but the feeder's (DESIGN.md
// 5.1).
//
// Here: the reader threads, the window pump both drivers run, run_index
// (dsx_index_*, dsx_cut_*) and run_ids (dsx_ids_*).  The arithmetic -- windows,
// pieces, shares, who hashes which chunk -- is dsx_index_plan.h, the host's
// share of the hashing dsx_hosttail.cpp.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <cerrno>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "dsx_engine.h"
#include "dsx_hosttail.h"
#include "dsx_index_plan.h"

namespace {

// Reads pieces [k*piece, (k+1)*piece) of the source into slot k % K on
// reader threads, ahead of the consumer, never more than K pieces ahead; from
// fine_from on (a multiple of piece) the pieces are `fine` bytes (PieceMap).
class Prefetcher {
 public:
  Prefetcher(FillFn fill, void* ud, uint64_t len, uint64_t piece, uint8_t* const* slots, int nslots,
             int nthreads, uint64_t fine_from = UINT64_MAX, uint64_t fine = 0)
      : fill_(fill), ud_(ud), map_(len, piece, fine_from, fine), np_(map_.np),
        slots_(slots, slots + nslots), have_(nslots, -1), allow_(nslots), rc_(nslots, 0) {
    for (int s = 0; s < nslots; ++s) allow_[s] = s;
    const int nt = std::max(1, std::min<int>(nthreads, (int)std::min<uint64_t>(np_, 64)));
    for (int i = 0; i < nt; ++i) th_.emplace_back([this] { run(); });
  }
  ~Prefetcher() { stop(); }
  // blocks until piece k is in its slot; returns the fill status
  int wait(uint64_t k, uint8_t** p, uint64_t* n) {
    const size_t s = k % slots_.size();
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return have_[s] == (int64_t)k; });
    *p = slots_[s];
    *n = map_.size(k);
    return rc_[s];
  }
  // the slot holding piece k may be refilled (its H2D copy has landed)
  void release(uint64_t k) {
    const size_t s = k % slots_.size();
    {
      std::lock_guard<std::mutex> lk(m_);
      allow_[s] = (int64_t)(k + slots_.size());
    }
    cv_.notify_all();
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
    th_.clear();
  }

 private:
  void run() {
    while (true) {
      uint64_t k;
      size_t s;
      {
        std::unique_lock<std::mutex> lk(m_);
        if (stop_ || next_ >= np_) return;
        k = next_++;
        s = k % slots_.size();
        cv_.wait(lk, [&] { return stop_ || allow_[s] == (int64_t)k; });
        if (stop_) return;
      }
      const int rc = fill_(ud_, slots_[s], map_.off(k), map_.size(k));
      {
        std::lock_guard<std::mutex> lk(m_);
        rc_[s] = rc;
        have_[s] = (int64_t)k;
      }
      cv_.notify_all();
    }
  }
  FillFn fill_;
  void* ud_;
  PieceMap map_;
  uint64_t np_;
  std::vector<uint8_t*> slots_;
  std::vector<int64_t> have_, allow_;
  std::vector<int> rc_;
  std::mutex m_;
  std::condition_variable cv_;
  uint64_t next_ = 0;
  bool stop_ = false;
  std::vector<std::thread> th_;
};

struct MemSrc {
  const uint8_t* p;
};
int fill_mem(void* ud, uint8_t* dst, uint64_t off, uint64_t n) {
  memcpy(dst, ((const MemSrc*)ud)->p + off, n);
  return DSX_OK;
}
struct FdSrc {
  int fd;
  uint64_t base;
};
int fill_fd(void* ud, uint8_t* dst, uint64_t off, uint64_t n) {
  const FdSrc* s = (const FdSrc*)ud;
  uint64_t got = 0;
  while (got < n) {
    const ssize_t r = pread(s->fd, dst + got, n - got, (off_t)(s->base + off + got));
    if (r < 0) {
      if (errno == EINTR) continue;
      return DSX_E_IO;
    }
    if (r == 0) return DSX_E_IO;  // the file shrank underneath us
    got += (uint64_t)r;
  }
  return DSX_OK;
}

int index_setup(dsx_ctx* c, uint64_t slot_bytes) {
  if (c->idx_slot_bytes < slot_bytes) {
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    for (auto& s : c->idx_slots) {
      if (s) (void)hipHostFree(s);
      s = nullptr;
    }
    c->idx_slot_bytes = 0;
    for (auto& s : c->idx_slots) HIPCHK(c, hipHostMalloc((void**)&s, slot_bytes));
    c->idx_slot_bytes = slot_bytes;
  }
  for (auto& e : c->idx_copy_ev)
    if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& e : c->idx_win_ev)
    if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& e : c->idx_stitch_ev)
    if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& s : c->idx_side)
    if (!s) HIPCHK(c, side_stream_create(&s));
  c->idx_dg_stream = c->idx_side[0];
  HIPCHK(c, c->idx_side_q.ensure(c->mem, 32 * (dsx_ctx::kIdxSide + 1)));  // (+ the end digest's)
  return DSX_OK;
}

// A window's digest on the digest stream, after the window's last stitch and
// snapshot (recorded on `stream`); then the event the copy stream waits for
// before it refills the window's buffer.
int launch_window_digest(dsx_ctx* c, const DigestArgs& da, uint64_t max_n, int algo, int slot,
                         uint32_t max_blocks = 0) {
  HIPCHK(c, hipEventRecord(c->idx_stitch_ev[slot], c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->idx_dg_stream, c->idx_stitch_ev[slot], 0));
  const int rc = launch_digest(c, da, max_n, algo, c->idx_dg_stream, nullptr, true, max_blocks);
  if (rc) return rc;
  HIPCHK(c, hipEventRecord(c->idx_win_ev[slot], c->idx_dg_stream));
  return DSX_OK;
}

// Drains both streams (after an error or a cancel: nothing may still read the
// pinned slots or the windows when the call returns).
int drain(dsx_ctx* c, Prefetcher& pf, int rc) {
  pf.stop();
  (void)hipStreamSynchronize(c->copy_stream);
  (void)hipStreamSynchronize(c->scan_stream);
  (void)hipStreamSynchronize(c->stream);
  for (auto& s : c->idx_side)  // (idx_dg_stream among them)
    if (s) (void)hipStreamSynchronize(s);
  return rc;
}

// Marks the progress of a run_index call (dsx_progress) for its lifetime.
struct ProgressScope {
  dsx_ctx* c;
  ProgressScope(dsx_ctx* cc, uint64_t len) : c(cc) {
    c->prog_active.store(0);
    c->prog_done.store(0);
    c->prog_len.store(len);
    ((volatile HostState*)c->h_state)->carry = 0;
    c->prog_active.store(1);
  }
  ~ProgressScope() { c->prog_active.store(0); }
  void set(uint64_t v) { c->prog_done.store(v); }
};

// The host tail's SHA threads, beside the readers within the process's CPU
// share (host_cpu_share: 16 on the GPU box, whose affinity mask shows the
// whole machine); the host's usual cut follows from them (feed_cut_for).
int feed_threads(const dsx_ctx* c) {
  int t = std::max(1, host_cpu_share() - c->index_readers);
#if DSX_DIAG
  if (const char* v = getenv("DSX_FEED_THREADS")) t = std::max(1, std::min(64, atoi(v)));
#endif
  return t;
}
// the host tail of a call's last window (SHA-512/256 only; auto needs AVX-512)
bool host_tail_on(const dsx_ctx* c, int algo) {
  return algo == DSX_DIGEST_SHA512_256 &&
         (c->index_host_tail > 0 || (c->index_host_tail < 0 && host_sha_vec()));
}

struct Ev {
  hipEvent_t e = nullptr;
  ~Ev() {
    if (e) (void)hipEventDestroy(e);
  }
};

#if DSX_DIAG
// (DSX_TAIL_LOG: the call's phases, to find which one a slow call spends its
// time in -- the reads, the wait for the host hash, the GPU)
using DiagClock = std::chrono::steady_clock;
double ms_since(DiagClock::time_point t0) {
  return std::chrono::duration<double, std::milli>(DiagClock::now() - t0).count();
}
bool tail_log() { return getenv("DSX_TAIL_LOG") != nullptr; }
#endif

// ---- the window pump ---------------------------------------------------------
// What run_index and run_ids share: the source's bytes [0, len) land piece by
// piece (the prefetcher's pinned slots, H2D on copy_stream) in two alternating
// HBM windows of g.W bytes, each with the last g.pre bytes of its predecessor
// in front.  The drivers decide what follows a piece (a scan, a share) and a
// window (its digest).
struct Landed {
  uint64_t n;      // the piece's bytes
  int fill_rc;     // the source's error reading it (nothing was enqueued), or
  hipError_t hip;  // a HIP error enqueueing its copy
};
struct Pump {
  static constexpr int K = dsx_ctx::kIdxSlots;
  dsx_ctx* c;
  Prefetcher& pf;
  WindowGeom g;
  uint64_t len;
  uint64_t k = 0;                  // the next piece
  uint64_t w = 0, ws = 0, wl = 0;  // the current window, its first byte and its length
  uint8_t* buf = nullptr;          // its buffer: g.pre bytes, then the window's

  // Window w_ becomes the current one: the copy stream waits for the digest
  // of window w_ - 2, which read this buffer, and copies the previous window's
  // last `pre` bytes (it was a full window) to the front.
  hipError_t begin_window(uint64_t w_) {
    w = w_;
    ws = w * g.W;
    wl = std::min(g.W, len - ws);
    buf = c->idx_win[w & 1].p;
    hipError_t e = hipSuccess;
    if (w >= 2) e = hipStreamWaitEvent(c->copy_stream, c->idx_win_ev[w & 1], 0);
    if (e == hipSuccess && w >= 1)
      e = hipMemcpyAsync(buf, c->idx_win[(w - 1) & 1].p + g.W, g.pre, hipMemcpyDeviceToDevice,
                         c->copy_stream);
    return e;
  }
  // The next piece, the source's bytes from `off` (in the current window),
  // lands: waits for its read (then after_read(its size)), enqueues its H2D
  // copy and the slot's event, and keeps two copies queued -- the previous
  // slot returns to the readers once its copy has landed.
  template <class AfterRead>
  Landed land(uint64_t off, AfterRead&& after_read) {
    uint8_t* hp = nullptr;
    uint64_t hn = 0;
    const int rc = pf.wait(k, &hp, &hn);
    if (rc) return {hn, rc, hipSuccess};
    after_read(hn);
    hipError_t e = hipMemcpyAsync(buf + g.pre + (off - ws), hp, hn, hipMemcpyHostToDevice, c->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(c->idx_copy_ev[k % K], c->copy_stream);
    if (e == hipSuccess && k >= 1) e = hipEventSynchronize(c->idx_copy_ev[(k - 1) % K]);
    if (e != hipSuccess) return {hn, DSX_OK, e};
    if (k >= 1) pf.release(k - 1);
    ++k;
    return {hn, DSX_OK, hipSuccess};
  }
  Landed land(uint64_t off) {
    return land(off, [](uint64_t) {});
  }
  // after the copy of the last piece landed (k >= 1)
  hipEvent_t last_copy_ev() const { return c->idx_copy_ev[(k - 1) % K]; }
  // A digest over the current window's bytes up to source offset `upto`:
  // window 0 starts at the source's byte 0, a later one `pre` bytes before
  // its own first byte.
  void window_args(DigestArgs& da, uint64_t upto) const {
    da.blob = w == 0 ? buf + g.pre : buf;
    da.base_off = w == 0 ? 0 : ws - g.pre;
    da.len = w == 0 ? upto : g.pre + (upto - ws);
  }
};

// ---- run_index ---------------------------------------------------------------
// One attempt of a run_index call: what its read loop, its shares, the end of
// its last window and an early return share.
struct IndexRun {
  dsx_ctx* c;
  const dsx_params_t* p;
  int algo;
  uint64_t len;
  uint64_t* out_ends;
  uint8_t* out_ids;
  uint64_t cap;
  uint64_t* n_out;
  const IndexGeom& g;
  const IndexSchedule& sc;  // the scan points, the shares that fire and every segment's cut
  const CallCfg& cc;
  ProgressScope& prog;
  Prefetcher& pf;
  Pump& pump;
  const TailSrc& tsrc;  // (the host tail's bytes)
  int fth;              // the feeder's threads
#if DSX_DIAG
  DiagClock::time_point call_t0;
#endif
  std::vector<Ev> mid_ev;  // share k's snapshot is in (recorded on `stream`)
  size_t mids_done = 0;    // shares fired
  // the last window's long chunks are hashed on the host during its read;
  // with several windows the feeder starts from the previous window's
  // snapshot (feed_ev: recorded after it)
  Ev feed_ev;
  std::unique_ptr<TailFeeder> feed;  // (last: it stops before its events go)
  std::vector<TailChunk> tail;       // the chunks the host hashed, and
  std::vector<uint8_t> tail_ids;     // their IDs

  // snapshot w: {cuts, carried cut} before window w; after the windows', share
  // k's: after the piece it fires at
  uint64_t* win_snap(uint64_t w) const { return c->idx_snap.p + 2 * w; }
  uint64_t* mid_snap(size_t k) const { return c->idx_snap.p + 2 * (g.nwin + 1 + k); }
  // the first side stream of the shares (several windows: the last one's
  // shares, on side streams 1.. -- side stream 0 carries the previous window's
  // digest meanwhile)
  size_t side0() const { return sc.side0; }
  // bounds a window's chunk count
  uint64_t window_max_n() const { return (g.pre + pump.wl) / p->min + 2; }
  // a digest of the chunk list over the current window's bytes up to `upto`
  DigestArgs window_digest(uint64_t upto) const {
    DigestArgs da{};
    pump.window_args(da, upto);
    da.ends = c->out.p;
    da.ids = c->dg_ids.p;
    return da;
  }
};

// Interrupted{} or a read error (make.go:133-162, :201-203): the chunks
// confirmed so far -- the chain up to the last stitched piece, a prefix
// of the true chain -- are returned with the error, IDs included: the
// current window's confirmed chunks are hashed first.
int index_partial(IndexRun& r, int err) {
  dsx_ctx* c = r.c;
  const uint64_t w = r.pump.w;
  drain(c, r.pf, err);
  // No piece of this call was scanned: the device chain state is another
  // call's, or in a fresh context was never written, and a snapshot of it
  // would send the digest over chunks that do not exist.
  if (c->init_pending) return err;
  if (r.algo >= 0) {
    hipLaunchKernelGGL(state_snapshot_kernel, dim3(1), dim3(64), 0, c->stream,
                       (const DevState*)c->state.p, r.win_snap(w + 1));
    DigestArgs da = r.window_digest(r.pump.ws + r.pump.wl);
    da.range_lo = r.win_snap(w);
    da.range_hi = r.win_snap(w + 1);
    if (launch_window_digest(c, da, r.window_max_n(), r.algo, (int)(w & 1))) return err;
  }
  HostState st;
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->idx_dg_stream);
  if (read_state(c, &st) || st.err) return err;  // (no piece stitched yet: nothing)
  const uint64_t n = std::min<uint64_t>(st.total, r.cap);
  if (n && hipMemcpy(r.out_ends, c->out.p, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return err;
  if (n && r.out_ids && hipMemcpy(r.out_ids, c->dg_ids.p, n * 32, hipMemcpyDeviceToHost) != hipSuccess)
    return err;
  *r.n_out = n;
  r.prog.set(n ? r.out_ends[n - 1] : 0);
  return err;
}

// One window (a file up to DSX_INDEX_WINDOW): the GPU hashes most of it
// DURING the read.  At the points f_k of the window (1/2, 3/4, ...) a
// snapshot follows the piece's stitch and a digest on side stream k (a
// "share") hashes the chunks confirmed since the previous point, all but
// those longer than cut_k = the read time left after f_k over the GPU's
// ns per byte (plan_shares): its chain ends about when the read does.  The feeder
// hashes, from the call's start, each segment's chunks above its cut and
// the last segment's above fcut_end; the digest after the read (on
// `stream`, digest_pc_kernel) takes the last segment's short chunks, a
// chain of at most fcut_end bytes.  The points stop where cut_k would
// fall below 1.5 x fcut (two points at 1 GiB and 12 threads); none
// when the first is below 2 x fcut (files below ~0.5 GiB), for
// SHA-256, or without the host tail.  At 1 GiB and 12 threads the host
// takes 2,985 chunks against 6,060 without the shares, and the call
// reads 0.87-0.90 x dsx_cut_fd against 0.78-0.84.
// The side streams have hardware queues of their own (side_stream_create):
// on one shared with the pipeline's streams the shares held the next
// pieces' scans and the call fell to 0.58-0.63 x dsx_cut_fd
// (profiles/r06q, r06x).  Four shares (down to 7/8 and 15/16) slowed the
// read: 0.87 against 0.89 (profiles/r06ag).
// (A first form gave the GPU every chunk of the first half and started
// the feeder at mid: the host then had less time for the same work, 0.66-
// 0.72 x dsx_cut_fd against 0.78, profiles/r06e, r06f.)
// (Which shares fire, at which scan point, and each segment's cut on
// both sides: index_schedule; the read loop executes it.)
//
// Fires the next share after the stitch of the piece that ends at `end`: the
// GPU's share of segment m, chunks [snap[m-1].total, snap[m].total) up to its
// cut, on 3/4 of the CUs (the rest keep room for the next pieces' scans).
// Returns the call's status: an error is drained already.
int index_fire_share(IndexRun& r, uint64_t end) {
  dsx_ctx* c = r.c;
  int share_pc = 1;
#if DSX_DIAG
  if (const char* v = getenv("DSX_SHARE_PC")) share_pc = atoi(v);
#endif
  const size_t m = r.mids_done++;
  const ShareSeg& seg = r.sc.segs[m];
  hipLaunchKernelGGL(state_snapshot_kernel, dim3(1), dim3(64), 0, c->stream,
                     (const DevState*)c->state.p, r.mid_snap(m));
  hipError_t e = hipEventRecord(r.mid_ev[m].e, c->stream);
  if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "index: record"));
  DigestArgs dm = r.window_digest(end);
  dm.range_lo = m ? r.mid_snap(m - 1) : r.win_snap(r.pump.w);
  dm.range_hi = r.mid_snap(m);
  dm.skip_above = seg.skip_above;
  // (on its own side stream after this stitch: the shares run side by side)
  hipStream_t ss = c->idx_side[r.side0() + m];
  e = hipStreamWaitEvent(ss, r.mid_ev[m].e, 0);
  if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "index: wait"));
  // (digest_pc_kernel: its chain ran ~45 ns/B during the read,
  // digest_kernel's ~85, profiles/r06aa, r06ab)
  const int rc = launch_digest(c, dm, (end - seg.from + 2 * r.p->max) / r.p->min + 2, r.algo, ss,
                               c->idx_side_q.p + 32 * (r.side0() + m), false, (uint32_t)(c->ncu * 3 / 4),
                               share_pc);
  if (rc) return drain(c, r.pf, rc);
  r.feed->add_boundary(r.mid_ev[m].e, r.mid_snap(m), r.sc.segs[m + 1].feed_cut);
#if DSX_DIAG
  if (tail_log())
    fprintf(stderr, "index: GPU share %zu up to %.1f MB (cut %lu), %.2f ms into the call\n", m, end / 1e6,
            (unsigned long)seg.feed_cut, ms_since(r.call_t0));
#endif
  return DSX_OK;
}

// The end of the last window with the host tail: `da` is the window's digest
// after the last stitch and snapshot, from the last fired share's snapshot.
// The host has the long chunks (r.tail, r.tail_ids), the GPU hashes the rest.
// Returns the call's status: an error is drained already, a cancel during
// the host hash has returned the confirmed chunks (index_partial).
int index_end_last_window(IndexRun& r, DigestArgs da) {
  dsx_ctx* c = r.c;
  const uint64_t w = r.pump.w;
  // the window's chunk ends (the stitch is done once the stream is)
  uint64_t snap[4];
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(snap, r.win_snap(w), sizeof snap, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "index: tail range"));
  const uint64_t i0 = snap[0], i1 = std::max(snap[0], snap[2]);
  std::vector<uint64_t> ends(i1 - i0);
  if (i1 > i0) e = hipMemcpy(ends.data(), c->out.p + i0, (i1 - i0) * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "index: tail ends"));
  int rc;
  if (r.feed) {  // the feeder has the long chunks: the GPU the rest
    // on `stream` after the last stitch (nothing follows it there; the
    // shares hold the side streams), sized by the count of the
    // window's chunks up to the cut, so that a window's ~10 K of them
    // run on digest_pc_kernel (its chain ~38 ns/B at the end of a call,
    // digest_kernel's ~58; profiles/r06aa)
    // (the last segment's cut, the one the feeder has used since the
    // last share that fired: index_schedule)
    const uint64_t fcut_end = r.sc.segs.back().feed_cut;
    da.skip_above = r.sc.segs.back().skip_above;
    uint64_t short_n = 0;
    for (uint64_t i = 0, st = snap[1]; i < ends.size(); st = ends[i++]) short_n += ends[i] - st <= fcut_end;
    // (its own queue counter: the previous window's digest may still
    // run on idx_dg_stream with the ctx's)
    rc = launch_digest(c, da, short_n + 2, r.algo, c->stream, c->idx_side_q.p + 32 * dsx_ctx::kIdxSide,
                       false);
    if (rc) return drain(c, r.pf, rc);
#if DSX_DIAG
    const auto tf0 = DiagClock::now();
    if (tail_log())
      fprintf(stderr, "feed: last piece stitched %.2f ms into the call\n", ms_since(r.call_t0));
#endif
    r.feed->finish(i1);
    rc = r.feed->join();
    if (rc == DSX_E_INTERRUPTED) return index_partial(r, rc);  // (dsx_cancel during the host hash)
    if (rc) return drain(c, r.pf, rc);
    r.tail = std::move(r.feed->chunks);
    r.tail_ids = std::move(r.feed->ids);
    c->stats.host_tail_chunks = r.tail.size();
#if DSX_DIAG
    if (tail_log()) {
      const double hms = ms_since(tf0);
      (void)hipStreamSynchronize(c->stream);
      const double gms = ms_since(tf0);
      for (size_t m = 0; m < r.mids_done; ++m) (void)hipStreamSynchronize(c->idx_side[r.side0() + m]);
      const double sms = ms_since(tf0);
      fprintf(stderr, "feed: chunks %lu host %zu (cut %lu) host done %.2f ms, GPU done %.2f ms, shares done %.2f ms\n",
              (unsigned long)i1, r.tail.size(), (unsigned long)fcut_end, hms, gms, sms);
    }
#endif
    return DSX_OK;
  }
  // (the end tail: reached only with the last-window feeder switched off,
  // DSX_FEED_MULTI=0 in the diagnostic build, the comparison of r05bt)
  const int threads = std::max(1, std::min(kTailThreads, host_cpu_share()));
  r.tail = plan_tail(c, ends, i0, snap[1], threads, &da.skip_above);
  rc = launch_window_digest(c, da, r.window_max_n(), r.algo, (int)(w & 1));
  if (rc) return drain(c, r.pf, rc);
  // the host's share while the GPU hashes the rest
  r.tail_ids.assign(32 * r.tail.size(), 0);
#if DSX_DIAG
  const auto th0 = DiagClock::now();
#endif
  if (!r.tail.empty()) rc = hash_tail(r.tsrc, r.tail, r.tail_ids.data(), threads, nullptr, &c->cancel);
  if (rc) return drain(c, r.pf, rc);
  c->stats.host_tail_chunks = r.tail.size();
#if DSX_DIAG
  if (tail_log()) {
    uint64_t hb = 0;
    for (const auto& x : r.tail) hb += x.len;
    const double hms = ms_since(th0);
    (void)hipStreamSynchronize(c->idx_dg_stream);
    const double gms = ms_since(th0);
    fprintf(stderr, "tail: window chunks %lu host %zu (%.1f MB, cut %lu) host %.2f ms, GPU done %.2f ms\n",
            (unsigned long)ends.size(), r.tail.size(), hb / 1e6, (unsigned long)da.skip_above, hms, gms);
  }
#endif
  return DSX_OK;
}

// The read loop of one attempt: executes the schedule window by window.
// `feeds`: the call has a host tail.  Returns the call's status: an error is
// drained already, a cancel or a read error has returned the confirmed chunks.
int index_read(IndexRun& r, bool feeds) {
  dsx_ctx* c = r.c;
  Pump& pump = r.pump;
  const IndexSchedule& sc = r.sc;
  const uint64_t len = r.len, pre = r.g.pre, nwin = r.g.nwin;
  // the readers' CPUs join the feeder's hashers once the reads are done
  int feed_extra = std::max(0, std::min(c->index_readers, host_cpu_share() - r.fth));
#if DSX_DIAG
  if (const char* v = getenv("DSX_FEED_EXTRA")) feed_extra = std::max(0, std::min(16, atoi(v)));
#endif
  size_t scans_done = 0;
  for (uint64_t w = 0; w < nwin; ++w) {
    HIPCHK(c, pump.begin_window(w));
    const uint64_t ws = pump.ws, wl = pump.wl;
    if (sc.feed_on && w + 1 == nwin)
      r.feed.reset(new TailFeeder(c, r.tsrc, len, sc.segs[0].feed_cut, r.fth, r.window_max_n(),
                                  c->piece_seq, nwin > 1 ? r.feed_ev.e : nullptr, r.win_snap(w),
                                  feed_extra));
    uint64_t scanned = ws;
    for (uint64_t off = ws; off < ws + wl;) {
      if (c->cancel.load()) return index_partial(r, DSX_E_INTERRUPTED);
      const uint64_t k = pump.k;  // this piece
      const Landed ld = pump.land(off, [&](uint64_t hn) {
        if (r.feed && off + hn == len) r.feed->reads_done();  // (the readers are idle now)
      });
      if (ld.fill_rc) return index_partial(r, ld.fill_rc);
      if (ld.hip != hipSuccess) return drain(c, r.pf, set_hip_err(c, ld.hip, "index: H2D"));
      off += ld.n;
      const uint64_t end = off;
      if (scans_done == sc.scan.size() || end != sc.scan[scans_done]) continue;
      ++scans_done;
      hipError_t e = scan_wait(c, c->idx_copy_ev[k % Pump::K]);  // (the stitch follows the scan)
      if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "index: wait"));
      const uint64_t halo = w == 0 ? scanned : pre + (scanned - ws);
      c->timing = false;  // (no event records between the pipeline's kernels)
      int rc = enqueue_piece(c, r.cc, pump.buf + pre + (scanned - ws), halo, scanned, end - scanned,
                             end == len);
      c->timing = true;
      if (rc) return drain(c, r.pf, rc);
      scanned = end;
      if (r.mids_done < sc.fired.size() && end == sc.fired[r.mids_done].at && r.feed) {
        rc = index_fire_share(r, end);
        if (rc) return rc;
      }
#if DSX_DIAG
      if (end == len && tail_log())
        fprintf(stderr, "index: last piece enqueued %.2f ms into the call\n", ms_since(r.call_t0));
#endif
    }
    // (the schedule's scan points end every window, and its shares have all fired)
    if (scanned != ws + wl || (w + 1 == nwin && r.mids_done != sc.fired.size())) {
      c->err = "index: the read loop left the schedule";
      return drain(c, r.pf, DSX_E_INTERNAL);
    }
    // the window's finished chunks: [snap[w].total, snap[w+1].total) from
    // snap[w].carry, all inside this window's bytes
    if (r.algo < 0) {  // cut list only (dsx_cut_host / dsx_cut_fd)
      hipError_t e = hipEventRecord(c->idx_win_ev[w & 1], c->stream);
      if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "index: record"));
      continue;
    }
    hipLaunchKernelGGL(state_snapshot_kernel, dim3(1), dim3(64), 0, c->stream,
                       (const DevState*)c->state.p, r.win_snap(w + 1));
    if (feeds && w + 2 == nwin) {  // (the last window's feeder starts from this snapshot)
      hipError_t e = hipEventRecord(r.feed_ev.e, c->stream);
      if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "index: record"));
    }
    DigestArgs da = r.window_digest(ws + wl);
    da.range_lo = r.mids_done ? r.mid_snap(r.mids_done - 1) : r.win_snap(w);  // (after the GPU's shares)
    da.range_hi = r.win_snap(w + 1);
    if (feeds && w + 1 == nwin) {
      const int rc = index_end_last_window(r, da);
      if (rc) return rc;
    } else {
      const int rc = launch_window_digest(c, da, r.window_max_n(), r.algo, (int)(w & 1));
      if (rc) return drain(c, r.pf, rc);
    }
  }
  return DSX_OK;
}

int run_index(dsx_ctx* c, const dsx_params_t* p, int algo, uint64_t len, FillFn fill, void* ud,
              uint64_t* out_ends, uint8_t* out_ids, uint64_t cap, uint64_t* n_out,
              const uint8_t* direct = nullptr) {
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  int rc = ensure_attr_walk(c);
  if (rc) return rc;
  *n_out = 0;
  c->stats.host_tail_chunks = 0;
  if (len == 0) return DSX_OK;  // empty file: no chunks (TestChunkerEmptyFile)
  const uint64_t need = len / p->min + 2;
  const bool feeds = out_ids && host_tail_on(c, algo);
  const IndexGeom g(len, p->max, c->index_slot, c->index_window, feeds);
  const int fth = feed_threads(c);
  // the scan points, the shares that fire and every segment's cut, for the
  // read loop, the feeder and the last digest alike
  const IndexSchedule sc = index_schedule(g, len, p->max, fth, c->index_host_tail, feeds);
  rc = index_setup(c, g.piece);
  if (rc) return rc;
  HIPCHK(c, grow(c, c->idx_win[0], g.pre + g.W));
  if (g.nwin > 1) HIPCHK(c, grow(c, c->idx_win[1], g.pre + g.W));
  HIPCHK(c, grow(c, c->idx_snap, 2 * (g.nwin + 1 + kIdxSide)));  // (+ the last window's share snapshots)
  HIPCHK(c, grow(c, c->out, need));
  if (algo >= 0) HIPCHK(c, grow(c, c->dg_ids, need * 32));

  ProgressScope prog(c, len);
  const TailSrc tsrc{fill, ud, direct};
#if DSX_DIAG
  const auto call_t0 = DiagClock::now();
#endif
  for (int attempt = 0; attempt < 2; ++attempt) {
    const CallCfg cc{p, len, 0, kRound, c->out.p, need, attempt == 1};
    rc = reset_state(c, 0);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->idx_snap.p, 0, 2 * sizeof(uint64_t), c->stream));  // {0 cuts, cut 0}
    Prefetcher pf(fill, ud, len, g.piece, c->idx_slots, Pump::K, c->index_readers, g.fine_from, g.fine);
    Pump pump{c, pf, g, len};
    IndexRun r{c, p, algo, len, out_ends, out_ids, cap, n_out, g, sc, cc, prog, pf, pump, tsrc, fth,
#if DSX_DIAG
               call_t0,
#endif
               std::vector<Ev>(sc.fired.size())};
    if (feeds) HIPCHK(c, hipEventCreateWithFlags(&r.feed_ev.e, hipEventDisableTiming));
    for (auto& x : r.mid_ev) HIPCHK(c, hipEventCreateWithFlags(&x.e, hipEventDisableTiming));
    rc = index_read(r, feeds);
    if (rc) return rc;
    pf.stop();
    HostState st;
    rc = read_state(c, &st);  // (the stitches)
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    HIPCHK(c, hipStreamSynchronize(c->idx_dg_stream));  // (the digests)
    for (size_t m = 0; m < r.mids_done; ++m) HIPCHK(c, hipStreamSynchronize(c->idx_side[sc.side0 + m]));
    if (rc) return rc;
    if (st.err & kErrDense) {  // rare: a lane overflowed its candidate slots
      c->stats.dense_fallbacks++;
      continue;
    }
    if (st.err) {
      c->err = "index: stitch error";
      return DSX_E_INTERNAL;
    }
#if DSX_DIAG
    if (tail_log()) fprintf(stderr, "index: done %.2f ms into the call\n", ms_since(call_t0));
#endif
    c->stats.chunks = st.total;
    c->stats.repaired_segments = st.repaired;
    c->stats.chunks_discarded = st.discarded;
    *n_out = st.total;
    if (st.total > cap) return DSX_E_CAPACITY;
    if (st.total) {
      HIPCHK(c, hipMemcpy(out_ends, c->out.p, st.total * 8, hipMemcpyDeviceToHost));
      if (out_ids) HIPCHK(c, hipMemcpy(out_ids, c->dg_ids.p, st.total * 32, hipMemcpyDeviceToHost));
      for (size_t j = 0; j < r.tail.size(); ++j)  // (the GPU skipped these)
        if (r.tail[j].idx < st.total) memcpy(out_ids + 32 * r.tail[j].idx, r.tail_ids.data() + 32 * j, 32);
    }
    prog.set(len);
    return DSX_OK;
  }
  c->err = "dense-candidate path overflowed";
  return DSX_E_INTERNAL;
}

// ---- run_ids -----------------------------------------------------------------
// The host's chunks of a run_ids call -- every segment's above its feed_cut
// (ids_schedule), longest first -- hashed on a thread from the call's start,
// beside the read; offsets relative to the list's start, as `src` reads them.
struct EarlyHash {
  std::vector<TailChunk> chunks;
  std::vector<uint8_t> ids;  // chunks[j]'s at 32 j, once join() returned DSX_OK
#if DSX_DIAG
  DiagClock::time_point t0 = DiagClock::now();
  double t_join0 = 0, t_join1 = 0;  // join() called and returned, ms after t0
#endif
  void start(const IdsSchedule& sc, uint64_t first, const uint64_t* ends, const TailSrc& src, int threads,
             const std::atomic<int>* cancel) {
    src_ = src;
    for (const IdSeg& seg : sc.segs)
      for (uint64_t i = seg.i_from; i < seg.i_to; ++i) {
        const uint64_t s0 = i ? ends[i - 1] - first : 0, e0 = ends[i] - first;
        if (e0 - s0 > seg.feed_cut) chunks.push_back({i, s0, e0 - s0});
      }
    std::sort(chunks.begin(), chunks.end(), [](const TailChunk& a, const TailChunk& b) { return a.len > b.len; });
    ids.assign(32 * chunks.size(), 0);
    if (!chunks.empty())
      t_ = std::thread([this, threads, cancel] { rc_ = hash_tail(src_, chunks, ids.data(), threads, &halt_, cancel); });
  }
  int join() {
#if DSX_DIAG
    t_join0 = ms_since(t0);
#endif
    if (t_.joinable()) t_.join();
#if DSX_DIAG
    t_join1 = ms_since(t0);
#endif
    return rc_;
  }
  ~EarlyHash() {  // (an error return stops the hash at its next group, then joins)
    halt_.store(1);
    if (t_.joinable()) t_.join();
  }

 private:
  TailSrc src_{};
  int rc_ = DSX_OK;
  std::atomic<int> halt_{0};
  std::thread t_;
};

// What run_ids's read loop and its shares share.
struct IdsRun {
  dsx_ctx* c;
  int algo;
  uint64_t start;
  const uint64_t* ends;
  const IdsSchedule& sc;  // the windows' ranges, the shares and every segment's cut
  Prefetcher& pf;
  Pump& pump;
  size_t shares_done = 0;
  // a digest of the list's chunks [a, b) (the list is on the device, relative to start)
  void list_range(DigestArgs& da, uint64_t a, uint64_t b) const {
    da.ends = c->dg_ends.p + a;
    da.first_start = a == 0 ? 0 : ends[a - 1] - start;
    da.n = b - a;
    da.ids = c->dg_ids.p + a * 32;
  }
};

// Fires the next share: its chunks' bytes have landed once the last piece's
// copy has.  On its side stream, on 3/4 of the CUs, digest_pc_kernel (as
// run_index's shares).  Returns the call's status: an error is drained already.
int ids_fire_share(IdsRun& r) {
  dsx_ctx* c = r.c;
  const size_t m = r.shares_done++;
  const IdSeg& seg = r.sc.segs[m];
  if (seg.i_to == seg.i_from) return DSX_OK;
  hipStream_t ss = c->idx_side[m];
  const hipError_t e = hipStreamWaitEvent(ss, r.pump.last_copy_ev(), 0);
  if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "ids: wait"));
  DigestArgs dm{};
  r.pump.window_args(dm, r.sc.shares[m].landed);
  r.list_range(dm, seg.i_from, seg.i_to);
  dm.skip_above = seg.skip_above;
  const int rc = launch_digest(c, dm, dm.n, r.algo, ss, c->idx_side_q.p + 32 * m, false,
                               (uint32_t)(c->ncu * 3 / 4), 1);
  return rc ? drain(c, r.pf, rc) : DSX_OK;
}

// The read loop: executes the schedule window by window.  `early`: the host's
// hash to join at the end of the last window (null: no host tail).  Returns
// the call's status: an error is drained already.
int ids_read(IdsRun& r, EarlyHash* early) {
  dsx_ctx* c = r.c;
  Pump& pump = r.pump;
  const IdsSchedule& sc = r.sc;
  uint64_t i0 = 0;
  for (uint64_t w = 0; w < sc.g.nwin; ++w) {
    HIPCHK(c, pump.begin_window(w));
    const uint64_t wend = pump.ws + pump.wl;
    for (uint64_t off = pump.ws; off < wend;) {
      if (c->cancel.load()) return drain(c, r.pf, DSX_E_INTERRUPTED);
      const Landed ld = pump.land(off);
      if (ld.fill_rc) return drain(c, r.pf, ld.fill_rc);
      if (ld.hip != hipSuccess) return drain(c, r.pf, set_hip_err(c, ld.hip, "ids: H2D"));
      off += ld.n;
      if (r.shares_done < sc.shares.size() && off >= sc.shares[r.shares_done].landed) {
        const int rc = ids_fire_share(r);
        if (rc) return rc;
      }
    }
    // the window's chunks [i0, i1) on `stream`, once its copies have landed
    // (then its buffer is free); the last window's: the last segment, the
    // chunks after the shares, less those the host has
    const bool last = w + 1 == sc.g.nwin;
    const uint64_t i1 = sc.win_i1[w];
    if (pump.k >= 1) {
      const hipError_t e = hipStreamWaitEvent(c->stream, pump.last_copy_ev(), 0);
      if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "ids: wait"));
    }
    DigestArgs da{};
    pump.window_args(da, wend);
    r.list_range(da, last ? sc.segs.back().i_from : i0, i1);
    if (last) da.skip_above = sc.segs.back().skip_above;
    if (i1 > i0 && da.n) {
      const int rc = launch_digest(c, da, da.n, r.algo);
      if (rc) return drain(c, r.pf, rc);
    }
    if (last && early) {
      const int rc = early->join();
      if (rc) return drain(c, r.pf, rc);
      c->stats.host_tail_chunks = early->chunks.size();
    }
    const hipError_t e = hipEventRecord(c->idx_win_ev[w & 1], c->stream);
    if (e != hipSuccess) return drain(c, r.pf, set_hip_err(c, e, "ids: record"));
    i0 = i1;
  }
  return DSX_OK;
}

// IDs of a given contiguous chunk list [start, ends[0]), [ends[0], ends[1]),
// ... of the source's bytes [0, len): the same reader / window pipeline as
// run_index without the scan.  The source is read from `start` to the last
// end; a window's halo is the longest chunk, so every chunk is hashed in the
// window where it ends, with all its bytes resident.  The ranges per window
// come from the host's list (no device snapshots).
//
// The list is known up front, so the host hashes the last window's long
// chunks from the call's start, beside the read (the tail feeder of run_index
// without the wait for the stitch), the GPU's shares take the shorter ones of
// their segments during the read, and that window's digest after the read the
// rest.  Who takes which chunk, and every cut: ids_schedule.
int run_ids(dsx_ctx* c, int algo, uint64_t len, FillFn fill, void* ud, uint64_t start,
            const uint64_t* ends, uint64_t n, uint8_t* out_ids, const uint8_t* direct = nullptr) {
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  if (n == 0) return DSX_OK;
  if (n > 0xFFFFFFF0ull) return DSX_E_INVAL;
  uint64_t prev = start, maxc = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (ends[i] < prev || ends[i] > len) {
      c->err = "chunk ends must be non-decreasing, start <= ends[0], ends[n-1] <= len";
      return DSX_E_INVAL;
    }
    maxc = std::max(maxc, ends[i] - prev);
    prev = ends[i];
  }
  // bytes [start, last) relative to `start` from here on
  const uint64_t L = ends[n - 1] - start;
  const WindowGeom g = window_geom(L, maxc, c->index_slot, c->index_window);
  int rc = index_setup(c, g.piece);
  if (rc) return rc;
  HIPCHK(c, grow(c, c->idx_win[0], g.pre + g.W));
  if (g.nwin > 1) HIPCHK(c, grow(c, c->idx_win[1], g.pre + g.W));
  HIPCHK(c, grow(c, c->dg_ends, n));
  HIPCHK(c, grow(c, c->dg_ids, n * 32));
  // the list, relative to `start`, on the device
  {
    std::vector<uint64_t> rel(n);
    for (uint64_t i = 0; i < n; ++i) rel[i] = ends[i] - start;
    HIPCHK(c, hipMemcpyAsync(c->dg_ends.p, rel.data(), n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  struct Shifted {
    FillFn fill;
    void* ud;
    uint64_t start;
  } sh{fill, ud, start};
  auto fill_shifted = [](void* u, uint8_t* dst, uint64_t off, uint64_t cnt) {
    const Shifted* s = (const Shifted*)u;
    return s->fill(s->ud, dst, s->start + off, cnt);
  };
  Prefetcher pf(fill_shifted, &sh, L, g.piece, c->idx_slots, Pump::K, c->index_readers);
  // (the readers have started: the plan over the list runs beside the first
  // reads.  This host's SHA rate is measured once per process, by the first
  // call that can have shares.)
  const bool tail_on = host_tail_on(c, algo);
  const int eth = feed_threads(c);
  const IdsSchedule sc =
      ids_schedule(start, ends, n, c->index_slot, c->index_window, eth, c->index_host_tail, dsx_ctx::kIdxSide,
                   tail_on, tail_on && c->index_host_tail < 0 ? host_ns_per_byte() : kHostNsPerByte);
  if (sc.g.pre != g.pre || sc.g.piece != g.piece || sc.g.W != g.W || sc.g.nwin != g.nwin) {
    c->err = "ids: the schedule's windows are not the call's";
    return drain(c, pf, DSX_E_INTERNAL);
  }
  EarlyHash early;
  c->stats.host_tail_chunks = 0;
  if (tail_on)
    early.start(sc, start, ends, TailSrc{fill_shifted, &sh, direct ? direct + start : nullptr}, eth, &c->cancel);
  Pump pump{c, pf, g, L};
  IdsRun r{c, algo, start, ends, sc, pf, pump};
  rc = ids_read(r, tail_on ? &early : nullptr);
  if (rc) return rc;
  pf.stop();
  HIPCHK(c, hipStreamSynchronize(c->copy_stream));
  for (size_t m = 0; m < r.shares_done; ++m) HIPCHK(c, hipStreamSynchronize(c->idx_side[m]));
  HIPCHK(c, hipMemcpyAsync(out_ids, c->dg_ids.p, n * 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
#if DSX_DIAG
  if (tail_log()) {
    uint64_t hb = 0;
    for (const auto& x : early.chunks) hb += x.len;
    fprintf(stderr, "ids: %.1f MB windows %lu reads+H2D done %.2f ms, early hash joined %.2f ms "
            "(waited %.2f; %zu chunks %.1f MB on %d threads, cut %lu, %zu shares, end cut %lu), GPU done %.2f ms\n",
            L / 1e6, (unsigned long)g.nwin, early.t_join0, early.t_join1, early.t_join1 - early.t_join0,
            early.chunks.size(), hb / 1e6, eth, (unsigned long)sc.early_cut, sc.shares.size(),
            (unsigned long)sc.end_cut, ms_since(early.t0));
  }
#endif
  for (size_t j = 0; j < early.chunks.size(); ++j)  // (the GPU skipped these)
    memcpy(out_ids + 32 * early.chunks[j].idx, early.ids.data() + 32 * j, 32);
  return DSX_OK;
}


}  // namespace

#if DSX_DIAG
// The plan a one-window dsx_index_* call of `len` bytes makes with the default
// host tail (-1, AVX-512) at `threads` feeder threads: the feeder's cut, the
// cut after the GPU's last share, and the shares {at, cut} (returns their
// count, at most cap); and the pieces it reads (off, size), for tests on the
// CPU (tests/test_host_logic.py).
extern "C" int dsx_diag_index_plan(uint64_t len, uint64_t max_chunk, int threads, uint64_t* fcut,
                                   uint64_t* fcut_end, uint64_t* at, uint64_t* cut, int cap) {
  *fcut = feed_cut_for(-1, threads);
  const std::vector<Mid> m = plan_shares(len, max_chunk, *fcut);
  *fcut_end = m.empty() ? *fcut : share_end_cut(*fcut);
  const int n = (int)std::min<size_t>(m.size(), (size_t)std::max(0, cap));
  for (int i = 0; i < n; ++i) {
    at[i] = m[i].at;
    cut[i] = m[i].cut;
  }
  return (int)m.size();
}
extern "C" uint64_t dsx_diag_index_pieces(uint64_t len, uint64_t max_chunk, uint64_t slot, uint64_t window,
                                          int feeds, uint64_t* off, uint64_t* size, uint64_t cap) {
  const IndexGeom g(len, max_chunk, slot, window, feeds != 0);
  const PieceMap pm(len, g.piece, g.fine_from, g.fine);
  for (uint64_t k = 0; k < pm.np && k < cap; ++k) {
    off[k] = pm.off(k);
    size[k] = pm.size(k);
  }
  return pm.np;
}
// The schedule run_index executes (index_schedule) for a SHA-512/256 call
// with IDs on an AVX-512 host (the tail feeder on unless host_tail is 0), at
// `threads` feeder threads.  scan[0, *n_scan): the scan points (at most
// scan_cap written).  at/cut/fire[k]: planned share k, absolute, and the scan
// point it fires at (0: dropped); returns their count (at most share_cap
// written).  seg[4 j ..]: {from, to, the feeder's cut, the GPU's skip_above}
// of the last window's segment j < *n_seg (at most seg_cap written).
// info: {the last window's start, the first side stream of the shares, the
// feeder's usual cut, the last segment's cut, the side streams}.
extern "C" int dsx_diag_index_schedule(uint64_t len, uint64_t max_chunk, uint64_t slot, uint64_t window,
                                       int threads, int64_t host_tail, uint64_t* scan,
                                       uint64_t scan_cap, uint64_t* n_scan, uint64_t* at, uint64_t* cut,
                                       uint64_t* fire, int share_cap, uint64_t* seg, int seg_cap,
                                       int* n_seg, uint64_t* info) {
  if (len == 0) return -1;
  const bool feeds = host_tail != 0;
  const IndexGeom g(len, max_chunk, slot, window, feeds);
  const IndexSchedule s = index_schedule(g, len, max_chunk, threads, host_tail, feeds);
  *n_scan = s.scan.size();
  for (uint64_t i = 0; i < s.scan.size() && i < scan_cap; ++i) scan[i] = s.scan[i];
  for (size_t k = 0; k < s.mids.size() && (int)k < share_cap; ++k) {
    at[k] = s.mids[k].at;
    cut[k] = s.mids[k].cut;
    fire[k] = s.fire[k];
  }
  *n_seg = (int)s.segs.size();
  for (size_t j = 0; j < s.segs.size() && (int)j < seg_cap; ++j) {
    seg[4 * j] = s.segs[j].from;
    seg[4 * j + 1] = s.segs[j].to;
    seg[4 * j + 2] = s.segs[j].feed_cut;
    seg[4 * j + 3] = s.segs[j].skip_above;
  }
  info[0] = s.last_ws;
  info[1] = s.side0;
  info[2] = s.fcut;
  info[3] = s.fcut_end;
  info[4] = (uint64_t)dsx_ctx::kIdxSide;
  return (int)s.mids.size();
}
// The schedule run_ids executes (ids_schedule) for the list start, ends[0, n)
// at `threads` host hashers and `host_ns` ns per byte, with the host tail on
// or off.  win_i1[0, *n_win): the windows' chunk ranges (at most win_cap
// written).  share[3 k ..]: {landed, cut, i1} of share k; returns their count
// (at most share_cap written).  seg[4 j ..]: {i_from, i_to, the host's cut,
// the GPU's skip_above} of segment j < *n_seg (at most seg_cap written).
// info: {pre, piece, W, L, maxc, the last window's first chunk, early_cut,
// end_cut}.
extern "C" int dsx_diag_ids_schedule(uint64_t start, const uint64_t* ends, uint64_t n, uint64_t slot,
                                     uint64_t window, int threads, int64_t host_tail, int sides,
                                     int tail_on, double host_ns, uint64_t* win_i1, uint64_t win_cap,
                                     uint64_t* n_win, uint64_t* share, int share_cap, uint64_t* seg,
                                     int seg_cap, int* n_seg, uint64_t* info) {
  uint64_t prev = start;
  for (uint64_t i = 0; i < n; prev = ends[i++])
    if (ends[i] < prev) return -1;
  const IdsSchedule s = ids_schedule(start, ends, n, slot, window, threads, host_tail, sides, tail_on != 0, host_ns);
  *n_win = s.win_i1.size();
  for (uint64_t w = 0; w < s.win_i1.size() && w < win_cap; ++w) win_i1[w] = s.win_i1[w];
  for (size_t k = 0; k < s.shares.size() && (int)k < share_cap; ++k) {
    share[3 * k] = s.shares[k].landed;
    share[3 * k + 1] = s.shares[k].cut;
    share[3 * k + 2] = s.shares[k].i1;
  }
  *n_seg = (int)s.segs.size();
  for (size_t j = 0; j < s.segs.size() && (int)j < seg_cap; ++j) {
    seg[4 * j] = s.segs[j].i_from;
    seg[4 * j + 1] = s.segs[j].i_to;
    seg[4 * j + 2] = s.segs[j].feed_cut;
    seg[4 * j + 3] = s.segs[j].skip_above;
  }
  const uint64_t v[8] = {s.g.pre, s.g.piece, s.g.W, s.L, s.maxc, s.i_last, s.early_cut, s.end_cut};
  std::copy(v, v + 8, info);
  return (int)s.shares.size();
}
// run_ids's host rate on this host (measured once per process; no GPU)
extern "C" double dsx_diag_host_ns_per_byte() { return host_ns_per_byte(); }
#endif

void index_release(dsx_ctx* c) {
  c->idx_dg_stream = nullptr;  // (idx_side[0])
  for (auto& s : c->idx_side)
    if (s) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s), s = nullptr;
  for (auto& e : c->idx_stitch_ev)
    if (e) (void)hipEventDestroy(e), e = nullptr;
  for (auto& s : c->idx_slots) {
    if (s) (void)hipHostFree(s);
    s = nullptr;
  }
  c->idx_slot_bytes = 0;
  for (auto& e : c->idx_copy_ev)
    if (e) (void)hipEventDestroy(e), e = nullptr;
  for (auto& e : c->idx_win_ev)
    if (e) (void)hipEventDestroy(e), e = nullptr;
}

static bool bad_algo(int algo) { return algo != DSX_DIGEST_SHA512_256 && algo != DSX_DIGEST_SHA256; }

extern "C" int dsx_index_fd(dsx_ctx_t* c, int fd, uint64_t off, uint64_t len, const dsx_params_t* p,
                            int algo, uint64_t* out_ends, uint8_t* ids, uint64_t cap,
                            uint64_t* n_out) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !p || !n_out || fd < 0 || (cap && (!out_ends || !ids)) || bad_algo(algo))
    return DSX_E_INVAL;
  if (len == UINT64_MAX) {
    // GetFileSize (ioctl_linux.go:63-84): lseek(SEEK_END) gives the size of
    // a regular file and of a block device alike
    const off_t end = lseek(fd, 0, SEEK_END);
    if (end < 0) return DSX_E_IO;
    len = (uint64_t)end > off ? (uint64_t)end - off : 0;
  }
  if (const int rc = chain_begin(c, ChainKind::kIndexFd)) return rc;
  FdSrc s{fd, off};
  const int rc = run_index(c, p, algo, len, fill_fd, &s, out_ends, ids, cap, n_out);
  c->cancel.store(0);  // a dsx_cancel() issued before or during this call ends here
  return rc;
}

// The cut list alone from a file or host memory: the same pipeline without
// the digests.
extern "C" int dsx_cut_fd(dsx_ctx_t* c, int fd, uint64_t off, uint64_t len, const dsx_params_t* p,
                          uint64_t* out_ends, uint64_t cap, uint64_t* n_out) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !p || !n_out || fd < 0 || (cap && !out_ends)) return DSX_E_INVAL;
  if (len == UINT64_MAX) {
    const off_t end = lseek(fd, 0, SEEK_END);
    if (end < 0) return DSX_E_IO;
    len = (uint64_t)end > off ? (uint64_t)end - off : 0;
  }
  if (const int rc = chain_begin(c, ChainKind::kCutFd)) return rc;
  FdSrc s{fd, off};
  const int rc = run_index(c, p, -1, len, fill_fd, &s, out_ends, nullptr, cap, n_out);
  c->cancel.store(0);
  return rc;
}

extern "C" int dsx_cut_host(dsx_ctx_t* c, const void* h_blob, uint64_t len, const dsx_params_t* p,
                            uint64_t* out_ends, uint64_t cap, uint64_t* n_out) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !p || !n_out || (len && !h_blob) || (cap && !out_ends)) return DSX_E_INVAL;
  if (const int rc = chain_begin(c, ChainKind::kCutHost)) return rc;
  MemSrc s{(const uint8_t*)h_blob};
  const int rc = run_index(c, p, -1, len, fill_mem, &s, out_ends, nullptr, cap, n_out);
  c->cancel.store(0);
  return rc;
}

extern "C" int dsx_index_host(dsx_ctx_t* c, const void* h_blob, uint64_t len, const dsx_params_t* p,
                              int algo, uint64_t* out_ends, uint8_t* ids, uint64_t cap,
                              uint64_t* n_out) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !p || !n_out || (len && !h_blob) || (cap && (!out_ends || !ids)) || bad_algo(algo))
    return DSX_E_INVAL;
  if (const int rc = chain_begin(c, ChainKind::kIndexHost)) return rc;
  MemSrc s{(const uint8_t*)h_blob};
  const int rc = run_index(c, p, algo, len, fill_mem, &s, out_ends, ids, cap, n_out, s.p);
  c->cancel.store(0);
  return rc;
}

// IDs of a given chunk list read from a file / host memory (VerifyIndex,
// verifyindex.go:13-79; ChopFile's NewChunkWithID check, chop.go:76-80,
// chunk.go:60-73).
extern "C" int dsx_ids_fd(dsx_ctx_t* c, int fd, uint64_t off, uint64_t len, uint64_t start,
                          const uint64_t* ends, uint64_t n, int algo, uint8_t* ids) {
  DSX_FLUSH_BEHIND(c);
  if (!c || fd < 0 || (n && (!ends || !ids)) || bad_algo(algo)) return DSX_E_INVAL;
  if (len == UINT64_MAX) {
    const off_t end = lseek(fd, 0, SEEK_END);
    if (end < 0) return DSX_E_IO;
    len = (uint64_t)end > off ? (uint64_t)end - off : 0;
  }
  FdSrc s{fd, off};
  const int rc = run_ids(c, algo, len, fill_fd, &s, start, ends, n, ids);
  c->cancel.store(0);
  return rc;
}

extern "C" int dsx_ids_host(dsx_ctx_t* c, const void* h_blob, uint64_t len, uint64_t start,
                            const uint64_t* ends, uint64_t n, int algo, uint8_t* ids) {
  DSX_FLUSH_BEHIND(c);
  if (!c || (len && !h_blob) || (n && (!ends || !ids)) || bad_algo(algo)) return DSX_E_INVAL;
  MemSrc s{(const uint8_t*)h_blob};
  const int rc = run_ids(c, algo, len, fill_mem, &s, start, ends, n, ids, s.p);
  c->cancel.store(0);
  return rc;
}
