// dsx_store.h -- the chunk store in HBM (dsx_store.hip): what a context holds
// for it.  Included by dsx_engine.h behind dsx_idset.h.
#pragma once

#include <stdint.h>

#include <vector>

struct dsx_ctx;

// A chunk store (include/dsx.h, dsx_store_t): a tightly packed arena of chunk
// bytes keyed by chunk ID.  Entry e is the e-th chunk appended that a prune has
// not removed: its ID is ids[32 e], its bytes arena[ends[e-1], ends[e])
// (ends[-1] = 0).  slots[s] is
// 0xFFFFFFFF (empty) or an entry number; the table has idset_table_cap(
// max_chunks) slots, so its load factor never exceeds 0.5.  Nothing is ever
// reallocated: the arena's address holds for the store's life.  chunks and
// bytes are host copies of the fill state, advanced after each accepted put or
// copy and set back by a prune.  broken: a prune failed between its first and its last
// write to the store, which is then neither the old nor the new one; every call
// but dsx_store_destroy refuses it (DSX_E_STATE).
struct dsx_store {
  dsx_ctx* ctx = nullptr;
  DevBuf<uint8_t> ids;     // max_chunks * 32 bytes
  DevBuf<uint64_t> ends;   // max_chunks words, cumulative
  DevBuf<uint32_t> slots;  // cap words
  DevBuf<uint8_t> arena;   // arena_bytes
  DevBuf<uint64_t> stamps; // max_chunks words, once tracked
  uint64_t max_chunks = 0, arena_bytes = 0, cap = 0, salt = 0;
  uint64_t chunks = 0, bytes = 0;
  uint64_t clock = 0;
  bool broken = false, tracked = false;
};

// What a kernel takes of a store, by value in its arguments: n entries, bytes
// of the arena used, mask = cap - 1.  The destination of a put or a copy is
// written through its view, so the pointers are not const; the kernels that
// only read a store take the same view.  Device side: store_find
// (dsx_idset_dev.h).
struct StoreView {
  uint8_t* ids;
  uint64_t* ends;
  uint32_t* slots;
  uint64_t n, mask, salt, bytes;
  uint8_t* arena;
};

// The stamp ++clock hands out.  The clock saturates: at UINT64_MAX (reached
// only through a caller's own stamp) every later use is stamped UINT64_MAX, so
// a stamp never wraps to the oldest value; such uses are ordered by entry number.
inline uint64_t next_stamp(const dsx_store* s) { return s->clock == UINT64_MAX ? UINT64_MAX : s->clock + 1; }

inline StoreView view_of(const dsx_store* s) {
  return StoreView{s->ids.p, s->ends.p, s->slots.p, s->chunks, s->cap - 1, s->salt, s->bytes, s->arena.p};
}

// The scratch of the store's calls.  Grows once, reused.  (The call's own ID
// table and the staged copies of host arguments are IdsetScratch's.)
struct StoreScratch {
  DevBuf<uint8_t> flag;               // put: new[i]; verify: mismatch[e]; prune: keep[e]
  DevBuf<unsigned long long> blk;     // put, prune: {chunks, bytes} per workgroup, then their prefix sums
  DevBuf<unsigned long long> tot;     // kStoreCounters words
  DevBuf<unsigned long long> segs;    // put: the new chunks, prune: the survivors, as AsmSeg records (3 words each)
  DevBuf<unsigned long long> offs, sizes;  // locate / resolve: staged outputs
  DevBuf<uint32_t> idx;               // resolve: the store segments' target positions
  DevBuf<uint8_t> vids;               // verify: the computed IDs
  DevBuf<uint8_t> pids;               // prune: the survivors' IDs, packed ...
  DevBuf<unsigned long long> pends;   // ... and their new ends (copied over the store's after the arena moved)
  DevBuf<uint8_t> bounce;             // prune: one window of the compacted arena
  DevBuf<uint32_t> srce;              // copy: the source store's entry number per ID
  DevBuf<unsigned long long> pstamps; // prune, evict of a tracked store: the survivors' stamps, packed
  // dsx_store_evict: pinned[e], the selection's state (kEvictSel words), one histogram of 256
  // {entries, bytes} pairs per pass, the boundary class's {entries, bytes} per workgroup,
  // the evicted IDs packed
  DevBuf<uint8_t> ev_pinned, ev_ids;
  DevBuf<unsigned long long> ev_sel, ev_hist, ev_blk;
  // dsx_read_ranges (dsx_read.hip): the staged ranges (3 words each), each range's first chunk,
  // its table slots as a prefix sum inside its workgroup, the workgroups' sums, the counters,
  // and the gather table (AsmSeg records)
  DevBuf<unsigned long long> rd_ranges, rd_pref, rd_blk, rd_tot, rd_segs;
  DevBuf<uint32_t> rd_first;
  std::vector<dsx_store*> live;       // the context's stores
};

// put: stored, stored_bytes, present, error word; prune: kept, kept_bytes,
// UINT64_MAX - the first removed byte's offset (0: none), -, moved, moved_bytes;
// copy: copied, copied_bytes, present, missing, first_missing; others: [0] a count
constexpr int kStoreCounters = 6;

// dsx_store_evict's selection state: the stamp bytes chosen so far (after the
// last pass: the cutoff stamp T), the needs not yet met by the entries below
// them, 1 if the unpinned entries cannot meet the needs, then the pin launch's sums
enum { kSelPrefix = 0, kSelNeedChunks, kSelNeedBytes, kSelFailed, kSelEvictable, kSelEvictableBytes,
       kSelPinned, kEvictSel };

void store_release(dsx_ctx* c);  // frees the live stores (dsx_ctx_destroy)
