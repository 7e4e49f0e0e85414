// dsx_idset.h -- chunk-ID sets on the device (dsx_idset.hip): what a context
// holds for them.  Included by dsx_engine.h behind DevBuf.
#pragma once

#include <stdint.h>

#include <vector>

struct dsx_ctx;

// A set of chunk IDs (include/dsx.h, dsx_idset_t): a device copy of the IDs
// and the open-addressing table built over them.  slots[s] is 0xFFFFFFFF
// (empty) or the lowest position of one ID in ids[]; cap is a power of two
// >= 2 n.  It belongs to the context that created it (its memory is counted
// in that context's device_bytes and its kernels ran on that context's
// stream) and dies with it.
struct dsx_idset {
  dsx_ctx* ctx = nullptr;
  DevBuf<uint8_t> ids;     // n * 32 bytes
  DevBuf<uint32_t> slots;  // cap words
  uint64_t n = 0, n_unique = 0, cap = 0;
  uint64_t salt = 0;       // hash key of this table
  // the seed's own classes (dsx_seed_plan): sclass[p] = the lowest position of
  // ids[p]'s ID, built by the first plan that uses the set and kept
  DevBuf<uint32_t> sclass;         // n words, or empty
  std::vector<uint32_t> h_sclass;  // its host copy
};

// dsx_dedup's scratch: the target's table, the staged copies of host (or
// misaligned device) arguments, and the counters.  Grows once, reused.
struct IdsetScratch {
  DevBuf<uint32_t> slots;
  DevBuf<uint8_t> ids;
  DevBuf<uint64_t> ends;
  DevBuf<uint32_t> first_pos, seed_pos;
  DevBuf<unsigned long long> tot;  // kIdsetCounters words
  std::vector<dsx_idset*> live;    // the context's sets
  // the read side (dsx_seed_plan, dsx_assemble: dsx_assemble.hip)
  DevBuf<uint8_t> is_null;         // one byte per target chunk
  DevBuf<uint64_t> asm_segs;       // the plan as the gather kernel reads it (3 words a segment)
  DevBuf<uint8_t> asm_store;       // the staged copy of host store bytes
  DevBuf<uint8_t> asm_stash;       // dsx_assemble_inplace: old bytes out of the way of a window's writes
};

// One segment as the gather kernel reads it (dsx_assemble.hip).
namespace dsx {
struct AsmSeg {
  unsigned long long dst_off, bytes;
  const uint8_t* src;  // null: zeros
};
static_assert(sizeof(AsmSeg) == 24, "three words a segment (IdsetScratch::asm_segs)");
}  // namespace dsx
// Enqueues assemble_kernel on the ctx stream over a segment table that is
// already on the device (ascending, non-overlapping dst_off), for the bytes
// [lo, hi) of d_out[0, out_len): the tiles that hold them.  No check, no wait:
// the caller has made both.
int assemble_launch(dsx_ctx* c, const dsx::AsmSeg* d_segs, uint64_t nsegs, void* d_out,
                    uint64_t out_len, uint64_t lo, uint64_t hi, bool unaligned);

constexpr int kIdsetCounters = 4;  // unique, in_seed, size - start, size_not_in_seed

void idset_release(dsx_ctx* c);  // frees the live sets (dsx_ctx_destroy)
