// dsx_known_geom.h -- the arithmetic of dsx_chunk_ids_known (dsx_known.hip,
// DESIGN.md 4.11) as pure functions: which bytes of a chunk its fingerprint
// reads, how the fingerprint mixes them, and how the bytes of the (chunk, entry)
// pairs are cut into the tiles of the compare.  Integer arithmetic only.  The
// kernels and tests/known_model.cpp compile the same functions, so
// tests/test_known_host.py checks on the CPU what the GPU runs.
#ifndef DSX_KNOWN_GEOM_H_
#define DSX_KNOWN_GEOM_H_
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSX_KNOWN_HD __host__ __device__ inline
#else
#define DSX_KNOWN_HD inline
#endif

namespace dsx_known {

constexpr uint64_t kTile = 65536;  // DSX_KNOWN_TILE: pair bytes one workgroup of the compare owns
constexpr uint32_t kTries = 4;     // DSX_KNOWN_TRIES: entries compared with one chunk at most
constexpr uint32_t kProbes = 64;   // DSX_KNOWN_PROBES: table slots an insert or a probe visits at most
constexpr uint32_t kWindow = 32;   // bytes of one fingerprint window

// The windows of a chunk of `size` bytes: its first min(size, 32) bytes, its
// last min(size, 32) bytes and, from 96 bytes on, the 32 bytes at size/2 - 16.
// They lie inside [0, size) and are 96 bytes at most; below 64 bytes the first
// two overlap, which costs nothing but reading a byte twice.
struct Windows {
  uint64_t off[3];
  uint32_t len[3];
  uint32_t n;
};

DSX_KNOWN_HD Windows known_windows(uint64_t size) {
  Windows w;
  const uint32_t e = size < kWindow ? (uint32_t)size : kWindow;
  w.off[0] = 0, w.len[0] = e;
  w.off[1] = size - e, w.len[1] = e;
  w.off[2] = 0, w.len[2] = 0;
  w.n = 2;
  if (size >= 3 * kWindow) {
    w.off[2] = size / 2 - kWindow / 2, w.len[2] = kWindow;
    w.n = 3;
  }
  return w;
}

DSX_KNOWN_HD uint64_t mix(uint64_t x) {  // splitmix64's finalizer, a bijection
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// h folded over the len bytes at q, eight at a time, little-endian, a short
// last word padded with zeros
DSX_KNOWN_HD uint64_t fold(uint64_t h, const uint8_t* q, uint32_t len) {
  for (uint32_t i = 0; i < len; i += 8) {
    uint64_t word = 0;
    const uint32_t m = len - i < 8 ? len - i : 8;
    for (uint32_t b = 0; b < m; ++b) word |= (uint64_t)q[i + b] << (8 * b);
    h = mix(h ^ word);
  }
  return h;
}

// The fingerprint of the `size` bytes at p: the size, then the windows' bytes.
// (The windows are named one by one: indexed in a loop, the struct would live
// in memory in a kernel.)
DSX_KNOWN_HD uint64_t fingerprint(const uint8_t* p, uint64_t size) {
  const Windows w = known_windows(size);
  uint64_t h = mix(size ^ 0x9E3779B97F4A7C15ull);
  h = fold(h, p + w.off[0], w.len[0]);
  h = fold(h, p + w.off[1], w.len[1]);
  if (w.n == 3) h = fold(h, p + w.off[2], w.len[2]);
  return h;
}

// The pairs of chunk j are cnt[j] <= kTries copies of its size[j] bytes, laid
// end to end from beg[j] on: beg[] is the exclusive prefix sum of cnt * size,
// non-decreasing.  A chunk without pairs or without bytes holds no pair byte.
//
// The chunk that holds pair byte x (x below the total): the last j with
// beg[j] <= x.  Its successor begins beyond x, so it holds at least one byte.
// The chunks' begins are read through Beg (an array on the host; two arrays
// added up in the kernel).
template <class Beg>
DSX_KNOWN_HD uint64_t chunk_at(const Beg& beg, uint64_t n, uint64_t x) {
  uint64_t l = 0, r = n;  // the number of chunks with beg <= x, minus one
  while (l < r) {
    const uint64_t m = l + ((r - l) >> 1);
    if (beg(m) <= x) l = m + 1;
    else r = m;
  }
  return l ? l - 1 : 0;
}

// What tile [lo, hi) takes of chunk j's pairs (begin b, cnt pairs of size
// bytes): of pair t the bytes [from, to) of the chunk, for t in [t0, t1].
struct Part {
  uint32_t t0, t1;     // first and last pair touched (t0 > t1: none)
  uint64_t from, to;   // the first pair starts at `from`, the last ends at `to`
};

DSX_KNOWN_HD Part part_of(uint64_t b, uint32_t cnt, uint64_t size, uint64_t lo, uint64_t hi) {
  Part p;
  p.t0 = 1, p.t1 = 0, p.from = p.to = 0;
  const uint64_t e = b + (uint64_t)cnt * size;
  const uint64_t x0 = lo > b ? lo : b, x1 = hi < e ? hi : e;
  if (size == 0 || x0 >= x1) return p;
  p.t0 = (uint32_t)((x0 - b) / size);
  p.from = (x0 - b) % size;
  p.t1 = (uint32_t)((x1 - 1 - b) / size);
  p.to = (x1 - 1 - b) % size + 1;
  return p;
}

// the bytes of pair t inside a part: [a, z) of the chunk
DSX_KNOWN_HD void pair_bytes(const Part& p, uint32_t t, uint64_t size, uint64_t* a, uint64_t* z) {
  *a = t == p.t0 ? p.from : 0;
  *z = t == p.t1 ? p.to : size;
}

}  // namespace dsx_known
#endif  // DSX_KNOWN_GEOM_H_
