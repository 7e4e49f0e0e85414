// dsx_evict_geom.h -- the bucket choice of dsx_store_evict's radix descent
// (dsx_store.hip) as a pure function, for the device and for the host
// (tests/evict_geom_model.cpp runs it under the host sanitizers).
//
// The descent looks for the stamp of the last entry of the shortest prefix, in
// ascending (stamp, entry number), whose chunks and bytes meet two needs.  One
// pass histograms one byte of the stamps of the entries that share the bytes
// chosen so far: 256 buckets of {entries, bytes}.  The prefix ends in the first
// bucket at which both running sums, the bucket included, reach the needs;
// every entry of a lower bucket belongs to the prefix, so the needs inside the
// chosen bucket are the needs less the sums below it (each at least 0: one need
// may be met long before the other).  At least one need is above 0 on entry
// (the caller handles the empty prefix), and then at least one stays above 0:
// the sums below the chosen bucket did not reach both.
#ifndef DSX_EVICT_GEOM_H_
#define DSX_EVICT_GEOM_H_
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSX_EVICT_HD __host__ __device__
#else
#define DSX_EVICT_HD
#endif

namespace dsx_evict {

constexpr int kBuckets = 256;

struct Pair {
  uint64_t count, bytes;
};

struct Choice {
  int bucket;                          // 0..255, or -1: all 256 buckets together do not reach the needs
  uint64_t below_count, below_bytes;   // the sums of the buckets below it
  uint64_t need_chunks, need_bytes;    // the needs inside it
};

// passes of the descent over stamps <= clock: the bytes the clock has, at least one
DSX_EVICT_HD inline int passes_of(uint64_t clock) {
  int p = 1;
  while (p < 8 && (clock >> (8 * p)) != 0) ++p;
  return p;
}

DSX_EVICT_HD inline Choice choose(const Pair* h, uint64_t need_chunks, uint64_t need_bytes) {
  Choice c;
  c.bucket = -1;
  c.below_count = c.below_bytes = 0;
  c.need_chunks = need_chunks;
  c.need_bytes = need_bytes;
  uint64_t count = 0, bytes = 0;
  for (int b = 0; b < kBuckets; ++b) {
    const uint64_t below_count = count, below_bytes = bytes;
    count += h[b].count;
    bytes += h[b].bytes;
    if (h[b].count == 0) continue;  // (an empty bucket ends no prefix)
    if (count >= need_chunks && bytes >= need_bytes) {
      c.bucket = b;
      c.below_count = below_count;
      c.below_bytes = below_bytes;
      c.need_chunks = need_chunks > below_count ? need_chunks - below_count : 0;
      c.need_bytes = need_bytes > below_bytes ? need_bytes - below_bytes : 0;
      return c;
    }
  }
  return c;
}

}  // namespace dsx_evict
#endif  // DSX_EVICT_GEOM_H_
