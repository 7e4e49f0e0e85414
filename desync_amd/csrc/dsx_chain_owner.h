// dsx_chain_owner.h -- who owns a context's chain state: the one rule that
// every chain call asks before it touches dsx_ctx::state and dsx_ctx::out.
// No HIP in here (tests/chain_owner_model.cpp enumerates it on the CPU under
// the host sanitizers); the contract is written down in include/dsx.h beside
// dsx_ctx_create, and in DESIGN.md 3 ("Who owns the chain state").
//
// A context has one DevState and one staging list.  Three protocols keep
// something in them across calls: a queued DSX_NO_SYNC call until its
// dsx_result (safe by construction: every call starts after the queue's
// kernels and each queued call publishes into its own pinned slot), a stream
// from dsx_stream_begin until it is finished (the carried chain between two
// batches lives in DevState), and a shard from dsx_shard_local until its
// resolve (the speculative cuts live in the staging list, their count in
// DevState).  So:
//   - a chain call on a context whose stream is unfinished is refused;
//   - dsx_stream_begin with uncollected queued calls is refused (dsx_result's
//     synchronous redo is a chain call and must never run inside a stream);
//   - every other chain call runs, and makes a shard that waits for its
//     resolve stale: resolve, resolve_async and collect then refuse it.
// Neutral calls never come here.
#ifndef DSX_CHAIN_OWNER_H_
#define DSX_CHAIN_OWNER_H_
#include <stdint.h>

#include <string>

#include "../../include/dsx.h"

namespace dsx_host {

enum class ChainKind : uint8_t {
  kCut,          // dsx_cut_device, synchronous (dsx_result's redo among them)
  kCutQueued,    // dsx_cut_device with DSX_NO_SYNC
  kMany,         // dsx_cut_device_many
  kCutHost,      // dsx_cut_host
  kCutFd,        // dsx_cut_fd
  kIndexHost,    // dsx_index_host
  kIndexFd,      // dsx_index_fd
  kShardLocal,   // dsx_shard_local (its own run owns the shard)
  kStreamBegin,  // dsx_stream_begin
  kStreamBatch,  // a batch of the context's own stream (never refused)
  kCount
};

inline const char* chain_kind_name(ChainKind k) {
  switch (k) {
    case ChainKind::kCut: return "dsx_cut_device";
    case ChainKind::kCutQueued: return "dsx_cut_device (DSX_NO_SYNC)";
    case ChainKind::kMany: return "dsx_cut_device_many";
    case ChainKind::kCutHost: return "dsx_cut_host";
    case ChainKind::kCutFd: return "dsx_cut_fd";
    case ChainKind::kIndexHost: return "dsx_index_host";
    case ChainKind::kIndexFd: return "dsx_index_fd";
    case ChainKind::kShardLocal: return "dsx_shard_local";
    case ChainKind::kStreamBegin: return "dsx_stream_begin";
    case ChainKind::kStreamBatch: return "a stream batch";
    default: return "?";
  }
}

// what the owner cannot see by itself: the stream's and the queue's state at
// the moment of the call (dsx_ctx::st, dsx_ctx::pend)
struct ChainView {
  bool stream_unfinished = false;  // dsx_stream_begin's predicate
  uint32_t queued = 0;             // DSX_NO_SYNC calls not collected yet
};

class ChainOwner {
 public:
  enum class Shard : uint8_t { kNone, kValid, kStale };

  // A chain call of kind k is about to start (its arguments were accepted;
  // nothing was launched or allocated).  DSX_OK: go on; what the call will
  // clobber is invalidated.  DSX_E_STATE: *why names the disturbed protocol
  // first ("stream: ...", "queued calls: ..."), and nothing changed.
  int begin(ChainKind k, const ChainView& v, std::string* why) {
    if (k != ChainKind::kStreamBatch) {
      if (v.stream_unfinished) {
        if (k == ChainKind::kStreamBegin)
          *why = "stream: a stream is already active on this context (dsx_stream_end it first)";
        else
          *why = std::string("stream: ") + chain_kind_name(k) +
                 " on a context whose stream is unfinished would replace the chain the stream "
                 "carries between its batches (finish or dsx_stream_end the stream, or use "
                 "another context)";
        return DSX_E_STATE;
      }
      if (k == ChainKind::kStreamBegin && v.queued > 0) {
        *why = "queued calls: dsx_stream_begin with uncollected DSX_NO_SYNC calls (collect them "
               "with dsx_result first)";
        return DSX_E_STATE;
      }
    }
    if (k == ChainKind::kShardLocal) {
      shard_ = Shard::kNone;  // (shard_ready() after its run)
      pending_ = false;
    } else if (shard_ == Shard::kValid) {
      shard_ = Shard::kStale;
      staled_by_ = k;
    }
    return DSX_OK;
  }

  // dsx_shard_local's run succeeded: the chain state is the shard's
  void shard_ready() {
    shard_ = Shard::kValid;
    pending_ = false;
  }

  // dsx_shard_resolve / dsx_shard_resolve_async may read the shard's state
  int resolve(std::string* why) const {
    if (shard_ == Shard::kValid) return DSX_OK;
    *why = stale_text(shard_ == Shard::kStale);
    return DSX_E_STATE;
  }
  // dsx_shard_resolve_async launched its emit
  void resolve_launched() { pending_ = true; }
  // dsx_shard_collect: an asynchronous resolve waits, and the shard is whole
  int collect(std::string* why) {
    if (!pending_) {
      *why = "shard: dsx_shard_collect without a dsx_shard_resolve_async";
      return DSX_E_STATE;
    }
    pending_ = false;
    if (shard_ == Shard::kValid) return DSX_OK;
    *why = stale_text(shard_ == Shard::kStale);
    return DSX_E_STATE;
  }

  Shard shard() const { return shard_; }
  bool shard_pending() const { return pending_; }

 private:
  std::string stale_text(bool stale) const {
    if (!stale) return "shard: no dsx_shard_local on this context";
    return std::string("shard: ") + chain_kind_name(staled_by_) +
           " ran on this context after dsx_shard_local and replaced the shard's cuts (start the "
           "round over with dsx_shard_local)";
  }
  Shard shard_ = Shard::kNone;
  bool pending_ = false;
  ChainKind staled_by_ = ChainKind::kCut;
};

}  // namespace dsx_host
#endif  // DSX_CHAIN_OWNER_H_
