// dsx_known.h -- chunk IDs by comparison with a store's bytes (dsx_known.hip):
// what a context holds for it.  Included by dsx_engine.h behind dsx_aead.h.
#pragma once

#include <stdint.h>

struct dsx_ctx;

// The scratch of a dsx_chunk_ids_known call.  Grows once, reused; the sketch
// (tab_*) is rebuilt by every call.
struct KnownScratch {
  DevBuf<unsigned long long> tab_fp;  // the sketch: a slot's fingerprint ...
  DevBuf<uint32_t> tab_ent;           // ... and its store entry (0xFFFFFFFF: empty)
  DevBuf<uint32_t> cand;              // n * DSX_KNOWN_TRIES: chunk j's candidate entries
  DevBuf<uint8_t> flag;               // n * DSX_KNOWN_TRIES: 1 where a pair's bytes differ
  DevBuf<uint8_t> cnt;                // n: candidates of chunk j; bit 7: it hit a bound
  DevBuf<uint8_t> take;               // n: 1 where the digest kernels hash chunk j
  DevBuf<unsigned long long> beg;     // n: pair bytes in front of chunk j inside its workgroup
  DevBuf<unsigned long long> blk;     // {pairs, pair bytes} per workgroup of the probe, then their prefix sums
  DevBuf<unsigned long long> rblk;    // the resolve's totals per workgroup
  DevBuf<unsigned long long> off;     // staged known_off
  DevBuf<unsigned long long> tot;     // kKnownCounters words
};

// pairs, pair bytes (the probe's scan); recognised, recognised bytes, hashed
// bytes, pairs that differed, chunks that hit a bound and were hashed (the
// resolve's scan); entries the sketch could not insert
constexpr int kKnownCounters = 8;
