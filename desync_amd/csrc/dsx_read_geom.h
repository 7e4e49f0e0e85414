// dsx_read_geom.h -- the geometry of a range read (dsx_read.hip, DESIGN.md
// 4.10) as pure functions: which chunks of an index a byte range touches, and
// what each (range, chunk) pair copies where.  Integer arithmetic only.  The
// count and emit kernels and the host's dsx_read_plan compile the same
// functions, so tests/test_read_host.py checks on the CPU what the GPU runs.
#ifndef DSX_READ_GEOM_H_
#define DSX_READ_GEOM_H_
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSX_READ_HD __host__ __device__ inline
#else
#define DSX_READ_HD inline
#endif

namespace dsx_read {

// The lowest i in [0, n] with ends[i] > pos (n: none): the chunk that holds
// byte pos of a blob whose chunk i is [ends[i-1], ends[i]).  Chunks of size 0
// hold no byte and are never the answer.  On a list that does not ascend the
// answer is still a number in [0, n]: every index read lies below n.
DSX_READ_HD uint64_t chunk_of(const uint64_t* ends, uint64_t n, uint64_t pos) {
  uint64_t l = 0, r = n;
  while (l < r) {
    const uint64_t m = l + ((r - l) >> 1);
    if (ends[m] > pos) r = m;
    else l = m + 1;
  }
  return l;
}

// The chunks [first, first + count) a range touches.  beyond: the range leaves
// [start, blob_end] (or off + len wraps); such a range, and one of length 0,
// touches nothing.
struct Span {
  uint64_t first, count;
  bool beyond;
};

DSX_READ_HD Span span_of(const uint64_t* ends, uint64_t start, uint64_t n, uint64_t off,
                         uint64_t len) {
  Span s;
  s.first = 0;
  s.count = 0;
  const uint64_t blob_end = n ? ends[n - 1] : start;
  s.beyond = off < start || len > UINT64_MAX - off || off + len > blob_end;
  if (s.beyond || len == 0) return s;
  const uint64_t first = chunk_of(ends, n, off), last = chunk_of(ends, n, off + len - 1);
  if (first >= n || last >= n || last < first) return s;  // (never on ascending ends)
  s.first = first;
  s.count = last - first + 1;
  return s;
}

// What chunk [cs, ce) gives range [off, off + len) -> dst_off: bytes may be 0
// (a chunk of size 0 between two others).  bad_ends: ce < cs, which ascending
// ends never show.  [dst_off, dst_off + bytes) always lies inside the range's
// window, also with bytes == 0 (the gather's table stays ascending), and
// whenever bytes > 0, chunk_off + bytes <= ce - cs.
struct Piece {
  uint64_t chunk_off, dst_off, bytes;
  bool bad_ends;
};

DSX_READ_HD Piece piece_of(uint64_t cs, uint64_t ce, uint64_t off, uint64_t len, uint64_t dst_off) {
  Piece p;
  p.chunk_off = p.bytes = 0;
  p.bad_ends = ce < cs;
  const uint64_t end = off + len;
  uint64_t lo = off > cs ? off : cs;
  if (lo > end) lo = end;
  p.dst_off = dst_off + (lo - off);
  const uint64_t hi = end < ce ? end : ce;
  if (p.bad_ends || hi <= lo) return p;
  p.chunk_off = lo - cs;
  p.bytes = hi - lo;
  return p;
}

}  // namespace dsx_read
#endif  // DSX_READ_GEOM_H_
