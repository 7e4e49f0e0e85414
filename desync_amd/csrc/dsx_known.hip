// dsx_known.hip -- chunk IDs by comparison: the chunks of a resident blob whose
// bytes a store of the same HBM already holds get that entry's ID without being
// hashed (make.go:223 followed by HasChunk inside chunkstorage.go:44-67, for a
// store that is memory and not a disk).  DESIGN.md 4.11.
//
// A chunk whose bytes equal a stored entry's bytes has that entry's ID, and
// comparing bytes is a streaming read where SHA is a serial chain.  Recognition
// is only an accelerator: whatever it gives up on is hashed by the digest
// kernels and looked up by ID, so ids[] and known_off[] are what dsx_chunk_ids
// and dsx_store_locate write whichever path produced them.
//
// A call is a fixed sequence of launches on the context's stream:
//   sketch   one lane per store entry: the fingerprint of its bytes (its size
//            and up to 96 bytes at three windows, dsx_known_geom.h) goes into a
//            scratch open-addressing table, fingerprint -> entry; equal
//            fingerprints take further slots;
//   probe    one lane per blob chunk: the same fingerprint from the blob, up to
//            DSX_KNOWN_TRIES entries of equal fingerprint and equal size as
//            the chunk's pairs, and the pairs' bytes as a prefix sum inside the
//            workgroup;
//   scan     the workgroups' sums become exclusive prefix sums (dsx_blockscan.h);
//   compare  one workgroup per DSX_KNOWN_TILE of pair bytes, its first chunk by
//            bisection over the prefix sums: 16 bytes a lane from both sides, a
//            plain store of 1 into the pair's flag where they differ;
//   resolve  one lane per chunk: the first pair without a difference gives the
//            entry's ID and arena offset, otherwise the chunk is marked in the
//            take mask; totals per workgroup, then the scan again;
//   (the host reads the totals: the one wait before the hashing)
//   digest   the digest kernels over the take mask (DigestArgs.take);
//   find     one lane per hashed chunk: store_find of its new ID.
// Every loop over table slots is bounded by DSX_KNOWN_PROBES.  An entry that
// finds no free slot within the bound is not recognisable; a chunk whose probe
// meets no empty slot within it, or more than DSX_KNOWN_TRIES candidates, and
// that none of its pairs recognises, is hashed.  Both count in `untried`.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "dsx_callargs.h"
#include "dsx_engine.h"
#include "dsx_idset_dev.h"
#include "dsx_known_geom.h"

namespace dsx {

constexpr int kKnownThreads = 256;
constexpr u64 kKnownTile = dsx_known::kTile;
constexpr uint32_t kKnownTries = dsx_known::kTries;
constexpr uint32_t kKnownProbes = dsx_known::kProbes;
static_assert(kKnownTile == DSX_KNOWN_TILE && kKnownTries == DSX_KNOWN_TRIES &&
                  kKnownProbes == DSX_KNOWN_PROBES,
              "include/dsx.h states the constants of dsx_known_geom.h");
static_assert(kKnownTile % (16 * kKnownThreads) == 0, "a tile is whole passes of the workgroup");
static_assert(kKnownTries < 128, "KnownScratch::cnt keeps bit 7 for the bound");

// the counters of a call (KnownScratch::tot)
enum : int {
  kKnPairs = 0,
  kKnBytes,       // these two: the total of the probe's scan
  kKnRecognised,  // these five: the total of the resolve's scan
  kKnRecBytes,
  kKnHashedBytes,
  kKnFalse,
  kKnUntried,
  kKnNoSlot,  // entries the sketch could not insert
};
static_assert(kKnNoSlot + 1 == kKnownCounters, "KnownScratch::tot");
constexpr int kKnResolveWords = 5;

struct KnownArgs {
  const uint8_t* blob;
  u64 len;
  const uint64_t* ends;
  u64 start, n;
  StoreView st;  // (only read)
  u64* tab_fp;
  uint32_t* tab_ent;
  u64 tmask;
  uint32_t* cand;
  uint8_t* flag;
  uint8_t* cnt;
  uint8_t* take;
  u64* beg;
  u64* blk;
  u64* rblk;
  u64* tot;
  uint8_t* ids;  // [n][32], 16-byte aligned
  u64* off;      // [n]
};

// chunk j as the blob holds it; ok: it lies inside the blob (device ends are
// not checked on the host)
struct KnChunk {
  u64 cs, size;
  bool ok;
};
__device__ __forceinline__ KnChunk chunk_of(const KnownArgs& a, u64 j) {
  const u64 cs = j ? a.ends[j - 1] : a.start, ce = a.ends[j];
  KnChunk c;
  c.ok = cs <= ce && ce <= a.len;
  c.cs = cs;
  c.size = c.ok ? ce - cs : 0;
  return c;
}

// entry e as the arena holds it
__device__ __forceinline__ KnChunk entry_of(const StoreView& st, u64 e) {
  const u64 lo = e ? st.ends[e - 1] : 0, hi = st.ends[e];
  KnChunk c;
  c.ok = lo <= hi && hi <= st.bytes;  // (always, in a store the library filled)
  c.cs = lo;
  c.size = c.ok ? hi - lo : 0;
  return c;
}

// One lane per store entry.
__global__ __launch_bounds__(kKnownThreads) void known_sketch_kernel(KnownArgs a) {
  const u64 e = (u64)blockIdx.x * kKnownThreads + threadIdx.x;
  bool lost = false;
  if (e < a.st.n) {
    const KnChunk c = entry_of(a.st, e);
    lost = true;
    if (c.ok) {
      const u64 fp = dsx_known::fingerprint(a.st.arena + c.cs, c.size);
      u64 s = fp & a.tmask;
      for (uint32_t step = 0; step < kKnownProbes; ++step, s = (s + 1) & a.tmask) {
        uint32_t cur = __hip_atomic_load(&a.tab_ent[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur != kEmpty) continue;
        cur = atomicCAS(&a.tab_ent[s], kEmpty, (uint32_t)e);
        if (cur == kEmpty) {
          a.tab_fp[s] = fp;  // (read by the next launch only)
          lost = false;
          break;
        }
      }
    }
  }
  const u64 bl = __ballot(lost);
  if ((threadIdx.x & 63) == 0 && bl) atomicAdd(&a.tot[kKnNoSlot], (u64)__popcll(bl));
}

// One lane per blob chunk.
__global__ __launch_bounds__(kKnownThreads) void known_probe_kernel(KnownArgs a) {
  const u64 j = (u64)blockIdx.x * kKnownThreads + threadIdx.x;
  uint32_t cnt = 0;
  u64 size = 0;
  if (j < a.n) {
    const KnChunk c = chunk_of(a, j);
    bool bound = false;
    if (c.ok) {
      size = c.size;
      const u64 fp = dsx_known::fingerprint(a.blob + c.cs, c.size);
      u64 s = fp & a.tmask;
      bool ended = false;
      for (uint32_t step = 0; step < kKnownProbes; ++step, s = (s + 1) & a.tmask) {
        const uint32_t e = a.tab_ent[s];
        if (e == kEmpty) {
          ended = true;
          break;
        }
        if (a.tab_fp[s] != fp || e >= a.st.n) continue;
        const KnChunk x = entry_of(a.st, e);
        if (!x.ok || x.size != size) continue;
        if (cnt < kKnownTries) {
          a.cand[kKnownTries * j + cnt] = e;
          a.flag[kKnownTries * j + cnt] = 0;
          ++cnt;
        } else {
          bound = true;
        }
      }
      bound = bound || !ended;
    }
    a.cnt[j] = (uint8_t)(cnt | (bound ? 0x80u : 0u));
  }
  u64 before[2], all[2];
  block_scan<kKnownThreads, 2>({(u64)cnt, (u64)cnt * size}, before, all);
  if (j < a.n) a.beg[j] = before[1];
  if (threadIdx.x == 0) {
    a.blk[2 * (u64)blockIdx.x] = all[0];
    a.blk[2 * (u64)blockIdx.x + 1] = all[1];
  }
}

typedef uint32_t kn_v4u __attribute__((ext_vector_type(4)));
typedef kn_v4u kn_v4u_unaligned __attribute__((aligned(1)));
#define DSX_KN_GLOBAL __attribute__((address_space(1)))
typedef const DSX_KN_GLOBAL uint8_t* kn_src_t;

__device__ __forceinline__ uint32_t diff16(const DSX_KN_GLOBAL kn_v4u* x, kn_src_t y) {
  const kn_v4u p = *x;
  const kn_v4u q = *(const DSX_KN_GLOBAL kn_v4u_unaligned*)y;
  return (p.x ^ q.x) | (p.y ^ q.y) | (p.z ^ q.z) | (p.w ^ q.w);
}

// The workgroup compares len bytes at x and y; a lane's answer is non-zero when
// a byte it read differs.  The body is 16 bytes a lane, aligned on x (y lies at
// any offset from it and is loaded unaligned); the head up to x's alignment
// and the tail go by bytes.  No byte outside [0, len) is read on either side.
__device__ __forceinline__ uint32_t compare_piece(kn_src_t x, kn_src_t y, u64 len) {
  const uint32_t tid = threadIdx.x;
  const u64 head = std::min<u64>(len, (16 - ((uintptr_t)x & 15)) & 15);
  const u64 nw = (len - head) >> 4;
  const u64 tail = (len - head) & 15;
  uint32_t d = 0;
  if (tid < head) d |= (uint32_t)(x[tid] ^ y[tid]);
  if (tid >= 64 && tid - 64 < tail) {  // (another wave than the head's)
    const u64 i = head + 16 * nw + (tid - 64);
    d |= (uint32_t)(x[i] ^ y[i]);
  }
  const DSX_KN_GLOBAL kn_v4u* xb = (const DSX_KN_GLOBAL kn_v4u*)(x + head);
  kn_src_t yb = y + head;
  u64 w = tid;
  for (; w + 3 * kKnownThreads < nw; w += 4 * kKnownThreads) {  // eight loads in flight per lane
    const uint32_t d0 = diff16(xb + w, yb + 16 * w);
    const uint32_t d1 = diff16(xb + w + kKnownThreads, yb + 16 * (w + kKnownThreads));
    const uint32_t d2 = diff16(xb + w + 2 * kKnownThreads, yb + 16 * (w + 2 * kKnownThreads));
    const uint32_t d3 = diff16(xb + w + 3 * kKnownThreads, yb + 16 * (w + 3 * kKnownThreads));
    d |= d0 | d1 | d2 | d3;
  }
  for (; w < nw; w += kKnownThreads) d |= diff16(xb + w, yb + 16 * w);
  return d;
}

// the pair bytes in front of chunk j
struct KnBeg {
  const u64* blk;
  const u64* beg;
  __device__ __forceinline__ u64 operator()(u64 j) const {
    return blk[2 * (j / kKnownThreads) + 1] + beg[j];
  }
};

// One workgroup per tile of pair bytes, striding over the tiles (their number
// is known on the device only).  Every writer of a flag writes 1: no atomics,
// and the flags are the same on every run.
__global__ __launch_bounds__(kKnownThreads) void known_compare_kernel(KnownArgs a) {
  const u64 total = a.tot[kKnBytes];
  const KnBeg beg{a.blk, a.beg};
  for (u64 lo = (u64)blockIdx.x * kKnownTile; lo < total; lo += (u64)gridDim.x * kKnownTile) {
    const u64 hi = std::min<u64>(lo + kKnownTile, total);
    for (u64 j = dsx_known::chunk_at(beg, a.n, lo); j < a.n; ++j) {
      const u64 b = beg(j);
      if (b >= hi) break;
      const uint32_t cnt = a.cnt[j] & 0x7Fu;
      if (!cnt) continue;
      const KnChunk c = chunk_of(a, j);
      const dsx_known::Part p = dsx_known::part_of(b, cnt, c.size, lo, hi);
      for (uint32_t t = p.t0; t <= p.t1 && t < cnt; ++t) {
        uint64_t from, to;
        dsx_known::pair_bytes(p, t, c.size, &from, &to);
        const u64 e = a.cand[kKnownTries * j + t];
        const u64 elo = e ? a.st.ends[e - 1] : 0;  // (the probe checked the entry's range and size)
        const uint32_t d = compare_piece((kn_src_t)a.blob + c.cs + from,
                                         (kn_src_t)a.st.arena + elo + from, to - from);
        if (d) a.flag[kKnownTries * j + t] = 1;
      }
    }
  }
}

// One lane per chunk.
__global__ __launch_bounds__(kKnownThreads) void known_resolve_kernel(KnownArgs a) {
  const u64 j = (u64)blockIdx.x * kKnownThreads + threadIdx.x;
  u64 v[kKnResolveWords] = {};
  if (j < a.n) {
    const KnChunk c = chunk_of(a, j);
    const uint32_t cb = a.cnt[j], cnt = cb & 0x7Fu;
    bool rec = false;
    for (uint32_t t = 0; t < cnt && !rec; ++t) {
      if (a.flag[kKnownTries * j + t]) {
        ++v[kKnFalse - kKnRecognised];
        continue;
      }
      const u64 e = a.cand[kKnownTries * j + t];
      const Id32 id = load_id(a.st.ids, e);
      uint4* o = reinterpret_cast<uint4*>(a.ids + 32 * j);
      o[0] = id.lo;
      o[1] = id.hi;
      a.off[j] = e ? a.st.ends[e - 1] : 0;
      rec = true;
    }
    a.take[j] = rec ? 0 : 1;
    if (rec) {
      v[kKnRecognised - kKnRecognised] = 1;
      v[kKnRecBytes - kKnRecognised] = c.size;
    } else {
      v[kKnHashedBytes - kKnRecognised] = c.size;
      v[kKnUntried - kKnRecognised] = cb >> 7;
    }
  }
  u64 w[kKnResolveWords];
#pragma unroll
  for (int k = 0; k < kKnResolveWords; ++k) w[k] = wave_sum(v[k]);
  block_totals_to<kKnownThreads, kKnResolveWords>(w, a.rblk);
}

// One lane per chunk: the arena offset of a chunk the digest kernels hashed.
__global__ __launch_bounds__(kKnownThreads) void known_find_kernel(KnownArgs a) {
  const u64 j = (u64)blockIdx.x * kKnownThreads + threadIdx.x;
  if (j >= a.n || !a.take[j]) return;
  const uint32_t e = store_find(a.st, load_id(a.ids, j));
  a.off[j] = e == kEmpty ? ~0ull : (e ? a.st.ends[e - 1] : 0);
}

}  // namespace dsx

using namespace dsx;

extern "C" int dsx_chunk_ids_known(dsx_ctx_t* c, const dsx_store_t* s, const void* d_blob,
                                   uint64_t len, uint64_t start, const uint64_t* ends, uint64_t n,
                                   int algo, void* ids, uint64_t* known_off,
                                   dsx_known_totals_t* totals, uint32_t flags) {
  const uint32_t f_ends = DSX_ENDS_DEVICE, f_out = DSX_OUT_DEVICE;
  if (!c) return DSX_E_INVAL;
  if (!s || !ids) return invalid(c, "the store or the IDs' buffer is missing");
  DSX_FLUSH_BEHIND(c);
  if (totals) *totals = dsx_known_totals_t{};
  // ---- every check comes before any device work ----------------------------------
  if ((flags & ~(f_ends | f_out)) != 0) return invalid(c, "unknown flag bit");
  if (algo != DSX_DIGEST_SHA512_256 && algo != DSX_DIGEST_SHA256)
    return invalid(c, "unknown digest");
  if (!owns(c, s)) return foreign_store(c, DSX_E_STATE);
  if (s->broken) return broken_store(c);
  if (n > kCallMaxN) return invalid(c, "more chunks than a call takes (0xFFFFFFF0)");
  if (n && (!d_blob || !ends)) return invalid(c, "the blob or the chunk ends are missing");
  if (!(flags & f_ends)) {
    uint64_t prev = start;
    for (uint64_t i = 0; i < n; ++i) {
      if (ends[i] < prev || ends[i] > len)
        return invalid(c, "chunk ends must be non-decreasing, start <= ends[0], ends[n-1] <= len");
      prev = ends[i];
    }
  }
  if (n == 0) return DSX_OK;

  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  KnownScratch& w = c->known;
  hipStream_t st = c->stream;
  // ---- stage ---------------------------------------------------------------------
  KnownArgs a{};
  a.blob = (const uint8_t*)d_blob;
  a.len = len;
  a.start = start;
  a.n = n;
  a.st = view_of(s);
  int rc = stage_ends(c, ends, n, (flags & f_ends) != 0, &a.ends);
  if (rc) return rc;
  a.ids = (uint8_t*)ids;
  if (!(flags & f_out) || !aligned(ids, 16)) {
    HIPCHK(c, grow(c, c->dg_ids, n * 32));
    a.ids = c->dg_ids.p;
  }
  a.off = (u64*)known_off;
  if (!known_off || !(flags & f_out) || !aligned(known_off, 8)) {
    HIPCHK(c, grow(c, w.off, n));
    a.off = w.off.p;
  }
  const uint64_t cap = idset_table_cap(s->chunks);
  const uint64_t nblk = (n + kKnownThreads - 1) / kKnownThreads;
  HIPCHK(c, grow(c, w.tab_fp, cap));
  HIPCHK(c, grow(c, w.tab_ent, cap));
  HIPCHK(c, grow(c, w.cand, n * kKnownTries));
  HIPCHK(c, grow(c, w.flag, n * kKnownTries));
  HIPCHK(c, grow(c, w.cnt, n));
  HIPCHK(c, grow(c, w.take, n));
  HIPCHK(c, grow(c, w.beg, n));
  HIPCHK(c, grow(c, w.blk, 2 * nblk));
  HIPCHK(c, grow(c, w.rblk, kKnResolveWords * nblk));
  HIPCHK(c, grow(c, w.tot, kKnownCounters));
  a.tab_fp = w.tab_fp.p;
  a.tab_ent = w.tab_ent.p;
  a.tmask = cap - 1;
  a.cand = w.cand.p;
  a.flag = w.flag.p;
  a.cnt = w.cnt.p;
  a.take = w.take.p;
  a.beg = w.beg.p;
  a.blk = w.blk.p;
  a.rblk = w.rblk.p;
  a.tot = w.tot.p;
  HIPCHK(c, hipMemsetAsync(w.tab_ent.p, 0xFF, cap * sizeof(uint32_t), st));
  HIPCHK(c, hipMemsetAsync(w.tot.p, 0, kKnownCounters * sizeof(u64), st));
  // ---- sketch, probe, compare, resolve ---------------------------------------------
  const dim3 tpb(kKnownThreads);
  if (s->chunks) {
    const uint32_t eblk = (uint32_t)((s->chunks + kKnownThreads - 1) / kKnownThreads);
    hipLaunchKernelGGL(known_sketch_kernel, dim3(eblk), tpb, 0, st, a);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(known_probe_kernel, dim3((uint32_t)nblk), tpb, 0, st, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(block_array_scan_kernel<2>, dim3(1), dim3(kArrayScanThreads), 0, st, w.blk.p,
                     (u64)nblk, w.tot.p + kKnPairs);
  HIPCHK(c, hipGetLastError());
  if (s->chunks) {
    // The pair bytes are at most DSX_KNOWN_TRIES times the blob's; the workgroups
    // stride over the tiles there are, at most 16 a CU resident at once.
    const uint64_t span = len - std::min<uint64_t>(start, len);
    const uint64_t most = (span / kKnownTile + 1) * kKnownTries;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(most, 16ull * c->ncu));
    hipLaunchKernelGGL(known_compare_kernel, dim3(grid), tpb, 0, st, a);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(known_resolve_kernel, dim3((uint32_t)nblk), tpb, 0, st, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(block_array_scan_kernel<kKnResolveWords>, dim3(1), dim3(kArrayScanThreads), 0,
                     st, w.rblk.p, (u64)nblk, w.tot.p + kKnRecognised);
  HIPCHK(c, hipGetLastError());
  // ---- the one wait before the hashing ---------------------------------------------
  u64 tot[kKnownCounters] = {};
  HIPCHK(c, hipMemcpyAsync(tot, w.tot.p, sizeof tot, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (tot[kKnRecognised] > n) {
    c->err = "more chunks recognised than there are";
    return DSX_E_INTERNAL;
  }
  const uint64_t hashed = n - tot[kKnRecognised];
  if (hashed) {
    DigestArgs da{};
    da.blob = a.blob;
    da.len = len;
    da.ends = a.ends;
    da.first_start = start;
    da.n = n;
    da.ids = a.ids;
    da.take = w.take.p;
    rc = launch_digest(c, da, n, algo, nullptr, nullptr, false, 0, -1, hashed);
    if (rc) return rc;
    hipLaunchKernelGGL(known_find_kernel, dim3((uint32_t)nblk), tpb, 0, st, a);
    HIPCHK(c, hipGetLastError());
  }
  if (a.ids != ids) HIPCHK(c, hipMemcpyAsync(ids, a.ids, n * 32, hipMemcpyDefault, st));
  if (known_off && a.off != (u64*)known_off)
    HIPCHK(c, hipMemcpyAsync(known_off, a.off, n * 8, hipMemcpyDefault, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (totals) {
    totals->chunks = n;
    totals->recognised = tot[kKnRecognised];
    totals->recognised_bytes = tot[kKnRecBytes];
    totals->hashed = hashed;
    totals->hashed_bytes = tot[kKnHashedBytes];
    totals->pairs = tot[kKnPairs];
    totals->compared_bytes = tot[kKnBytes];
    totals->fp_false = tot[kKnFalse];
    totals->untried = tot[kKnUntried] + tot[kKnNoSlot];
  }
  return DSX_OK;
}
