// dsx_hosttail.h -- the host's share of the file pipeline's chunk IDs
// (dsx_hosttail.cpp; used by dsx_index.cpp): the long chunks of a call's last
// window hashed on the host (AVX-512 SHA-512/256) while the GPU hashes the
// rest.
#ifndef DSX_HOSTTAIL_H_
#define DSX_HOSTTAIL_H_
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "dsx_engine.h"

// a call's source: n bytes at offset off into dst; DSX_OK or an error
using FillFn = int (*)(void* ud, uint8_t* dst, uint64_t off, uint64_t n);

// The last window's digest starts when the read ends and lasts its longest
// chunk's SHA chain: ~38 ns per byte on one GPU lane, ~10 ms for 256 KiB.
// The longest chunks of that window go to the host instead (AVX-512, 8 per
// core at once), the GPU skipping them (DigestArgs.skip_above): the cut L is
// where the host's bytes over its threads take as long as the GPU's longest
// remaining chain.
// (measured at the end of a 1 GiB file call, profiles/r05ao: the GPU's chain
// runs at the clock an idle-ish GPU has then, ~58 ns per byte, against ~38 ns
// on a busy one; 16 host threads read and hash ~43 GB/s)
constexpr double kGpuNsPerByte = 58.0;   // digest_pc_kernel, one lane, end of a file call
constexpr double kHostNsPerByte = 0.38;  // one host thread, read + hash (AVX-512)
constexpr double kTailMinGainNs = 5e5;   // worth a host pass only above this
constexpr int kTailThreads = 16;

// This host's SHA-512/256 rate, ns per byte on one thread (8 lanes of 128 KiB
// hashed once per process, ~0.5 ms), plus the read: the VerifyIndex budget
// takes the slower of it and kHostNsPerByte, so a slower host gets fewer
// bytes instead of a call that waits for its early hash.
double host_ns_per_byte();

struct TailChunk {
  uint64_t idx, start, len;
};

// The chunks of ranges [i0, i1) (ends e, the first starting at first) that the
// host hashes, longest first; empty: none.  *cut = the GPU's skip_above.
std::vector<TailChunk> plan_tail(const dsx_ctx* c, const std::vector<uint64_t>& e, uint64_t i0,
                                 uint64_t first, int threads, uint64_t* cut);

// Where the host tail takes a chunk's bytes: straight from the caller's
// memory (dsx_*_host), else read again through the call's fill function
// (dsx_*_fd: the pages the readers just brought into the page cache).
// (Taking them from the pinned read slots instead, each slot kept three
// pieces longer for the feeder, saved the copy of ~0.7 GB per GiB and
// measured no gain, in-process A/B at three cuts, profiles/r06n/: the SHA
// rounds, not the copy, hold the host threads.)
struct TailSrc {
  FillFn fill;
  void* ud;
  const uint8_t* direct = nullptr;  // the source's bytes [0, len) in host memory
};

// Hashes chunks t[0, cnt) (cnt <= 8: one AVX-512 group, else cnt == 1 on the
// scalar path) into ids[32 j]; their bytes from the caller's memory or read
// again through `fill` into buf.
int hash_group(const TailSrc& src, const TailChunk* t, uint64_t cnt, uint8_t* ids,
               std::vector<uint8_t>& buf);

// Hashes the planned chunks into ids[32 j] for t[j]; 8 at a time per thread.
// Stops with DSX_E_INTERRUPTED between groups once `halt` (the caller's: a
// feeder told to stop, an error path joining it) or `cancel` (dsx_cancel) is
// set, so a cancelled call does not wait for a whole window's host hash.
int hash_tail(const TailSrc& src, const std::vector<TailChunk>& t, uint8_t* ids, int threads,
              const std::atomic<int>* halt, const std::atomic<int>* cancel);

// The long chunks of a call's last window (the whole file up to the window
// size) hashed on the host while that window is still being read: a thread
// follows the chain state each stitch publishes (HostState.total, seq written
// last), copies the newly final cut ends to the host and hashes the chunks
// longer than `cut` (read again through the call's fill function) on the host
// pool.  After the read, the GPU digest skips those chunks
// (DigestArgs.skip_above = cut) and hashes the rest, a chain of at most `cut`
// bytes; finish() hands the feeder the final count.
class TailFeeder {
 public:
  // (the last of several windows: start_ev marks the previous window's
  // snapshot dsnap = {cuts before this window, their last end})
  // (`cut`: the cut of the chunks before the first boundary; a boundary, a
  // snapshot the GPU hashed the shorter chunks before during the read, sets
  // the cut of those after it)
  // (cap: at most this many chunks in the window; extra: hashers that join
  // once reads_done() -- the readers' CPUs)
  TailFeeder(dsx_ctx* c, const TailSrc& src, uint64_t len, uint64_t cut, int threads, uint64_t cap,
             uint64_t seq0, hipEvent_t start_ev = nullptr, const uint64_t* dsnap = nullptr,
             int extra = 0)
      : c_(c), src_(src), len_(len), cut_(cut), cap_(cap), threads_(threads), extra_(extra),
        seq0_(seq0), start_ev_(start_ev), dsnap_(dsnap) {
    th_ = std::thread([this] { run(); });
  }
  // a snapshot {total, carry} was enqueued (ev after it): chunks from its
  // total on take `cut_after`.  Called before the pieces after the snapshot
  // are enqueued, so no total the feeder reads after it can come from them
  // without it knowing the boundary.
  void add_boundary(hipEvent_t ev, const uint64_t* snap, uint64_t cut_after) {
    std::lock_guard<std::mutex> g(m_);
    bounds_.push_back({ev, snap, cut_after, 0});
  }
  ~TailFeeder() { stop(); }
  // the call's reads are done: the extra hashers start
  void reads_done() { reads_done_.store(1); }
  void finish(uint64_t total);
  // joins; the hashed chunks and their IDs, or an error
  int join() {
    if (th_.joinable()) th_.join();
    return err_;
  }
  void stop();
  std::vector<TailChunk> chunks;
  std::vector<uint8_t> ids;

 private:
  // cuts the device has published as final, 0 if none of this call yet
  uint64_t published() const;
  void run();
  // the follower: each batch of newly final chunks above their cut goes to
  // `put` (which returns non-zero to stop); returns a HIP error, or OK once
  // the final count is in
  template <class Put>
  int produce(hipStream_t s, Put&& put);
  dsx_ctx* c_;
  TailSrc src_;
  uint64_t len_;
  uint64_t cut_, cap_;
  struct Bound {
    hipEvent_t ev;
    const uint64_t* snap;
    uint64_t cut_after, total;
  };
  std::vector<Bound> bounds_;  // (add_boundary, under m_)
  int threads_, extra_;
  std::atomic<int> reads_done_{0};
  uint64_t seq0_;
  hipEvent_t start_ev_;
  const uint64_t* dsnap_;
  std::thread th_;
  std::mutex m_;
  std::condition_variable cv_;
  bool stop_ = false, have_final_ = false;
  std::atomic<int> halt_{0};
  uint64_t final_ = 0;
  int err_ = DSX_OK;
};

#endif  // DSX_HOSTTAIL_H_
