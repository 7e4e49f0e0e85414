// dsx_store.h -- the chunk store in HBM (dsx_store.hip): what a context holds
// for it.  Included by dsx_engine.h behind dsx_idset.h.
#pragma once

#include <stdint.h>

#include <vector>

struct dsx_ctx;

// A chunk store (include/dsx.h, dsx_store_t): an append-only arena of chunk
// bytes keyed by chunk ID.  Entry e is the e-th chunk appended: its ID is
// ids[32 e], its bytes arena[ends[e-1], ends[e]) (ends[-1] = 0).  slots[s] is
// 0xFFFFFFFF (empty) or an entry number; the table has idset_table_cap(
// max_chunks) slots, so its load factor never exceeds 0.5.  Nothing is ever
// reallocated: the arena's address holds for the store's life.  chunks and
// bytes are host copies of the fill state, advanced after each accepted put.
struct dsx_store {
  dsx_ctx* ctx = nullptr;
  DevBuf<uint8_t> ids;     // max_chunks * 32 bytes
  DevBuf<uint64_t> ends;   // max_chunks words, cumulative
  DevBuf<uint32_t> slots;  // cap words
  DevBuf<uint8_t> arena;   // arena_bytes
  uint64_t max_chunks = 0, arena_bytes = 0, cap = 0, salt = 0;
  uint64_t chunks = 0, bytes = 0;
};

// The scratch of the store's calls.  Grows once, reused.  (The call's own ID
// table and the staged copies of host arguments are IdsetScratch's.)
struct StoreScratch {
  DevBuf<uint8_t> flag;               // put: new[i]; verify: mismatch[e]
  DevBuf<unsigned long long> blk;     // put: {chunks, bytes} per workgroup, then their prefix sums
  DevBuf<unsigned long long> tot;     // kStoreCounters words
  DevBuf<unsigned long long> segs;    // put: the new chunks as AsmSeg records (3 words each)
  DevBuf<unsigned long long> offs, sizes;  // locate / resolve: staged outputs
  DevBuf<uint32_t> idx;               // resolve: the store segments' target positions
  DevBuf<uint8_t> vids;               // verify: the computed IDs
  std::vector<dsx_store*> live;       // the context's stores
};

constexpr int kStoreCounters = 4;  // stored, stored_bytes, present, error word (put); [0]: a count (others)

uint64_t store_device_bytes(const dsx_ctx* c);  // scratch + live stores
void store_release(dsx_ctx* c);                 // frees both (dsx_ctx_destroy)
