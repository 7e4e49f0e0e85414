// dsx_read.hip -- byte ranges of an indexed blob read out of a chunk store in
// HBM (readseeker.go: NewIndexReadSeeker, IndexPos.Read; cmd/desync/cat.go's
// -o / -l; mount-index): many ranges a call, without the index, the store's
// offsets or a segment list crossing to the host.  The read-side counterpart
// of dsx_cut_device_many; DESIGN.md 4.10.
//
// A call is a fixed sequence of launches on the context's stream:
//   count   one lane per range: its first and last chunk by bisection over the
//           chunk ends (dsx_read_geom.h), the number of table slots it takes
//           (one per chunk from the first to the last) as a prefix sum inside
//           its workgroup, and whether it leaves the blob;
//   scan    one workgroup turns the workgroups' sums into exclusive prefix sums
//           and leaves the total (the store's scan, dsx_blockscan.h), so range r's
//           slots are a contiguous, ascending slice of the table;
//   emit    work is divided by slots, not by ranges: a lane finds its slot's
//           range by bisection over the prefix sums, its chunk from the range's
//           first, clips the chunk to the range, compares the chunk's ID with
//           the null ID, else probes the store's ID table, compares the sizes
//           and writes the gather record (arena address + chunk_off, or a null
//           source for zeros).  Errors are counted per wave by ballot, the
//           lowest bad range and chunk found with atomicMin;
//   (the host reads the counters: anything missing, of another size or beyond
//   the blob ends the call here, before a byte of the output is written)
//   gather  assemble_kernel (dsx_assemble.hip) over the table.
// The table's size is not known before the scan when the ends are device
// memory, so the emit takes the table's capacity and gives up (a flag, nothing
// written past the capacity) when the total exceeds it; the host then grows the
// table and runs the emit again.  A context's second call of a shape never does.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dsx_callargs.h"
#include "dsx_engine.h"
#include "dsx_idset_dev.h"
#include "dsx_read_geom.h"

namespace dsx {

constexpr int kReadThreads = 256;
constexpr u64 kNone = ~0ull;

// the counters of a call (rd_tot)
enum : int {
  kRdPieces = 0,
  kRdStoreBytes,
  kRdNullBytes,
  kRdMissing,
  kRdWrong,
  kRdBeyond,
  kRdBadRange,  // starts at kNone
  kRdBadChunk,  // starts at kNone
  kRdSlots,     // written by the scan
  kRdOverflow,  // the emit: the table is too small for kRdSlots
  kRdCounters
};

struct ReadArgs {
  const u64* ranges;  // {off, len, dst_off} per range
  u64 nranges;
  const uint8_t* ids;  // the index
  const uint64_t* ends;
  u64 start, n;
  Id32 null_id;
  u64 has_null, null_size;
  StoreView st;     // the store (only read)
  u64* pref;        // [nranges] slots of the ranges before r in r's workgroup
  uint32_t* first;  // [nranges] the first chunk of range r
  u64* blk;         // [workgroups of the count] their slots, then the exclusive prefix sums
  u64 nblk;
  u64* tot;  // [kRdCounters]
  AsmSeg* segs;
  u64 cap;  // records segs[] holds
};

// One lane per range.
__global__ __launch_bounds__(kReadThreads) void read_count_kernel(ReadArgs a) {
  const u64 r = (u64)blockIdx.x * kReadThreads + threadIdx.x;
  u64 cnt = 0;
  bool beyond = false;
  if (r < a.nranges) {
    const dsx_read::Span s =
        dsx_read::span_of(a.ends, a.start, a.n, a.ranges[3 * r], a.ranges[3 * r + 1]);
    beyond = s.beyond;
    cnt = s.count;
    a.first[r] = (uint32_t)s.first;
  }
  const u64 bb = __ballot(beyond);
  if ((threadIdx.x & 63) == 0 && bb) {
    atomicAdd(&a.tot[kRdBeyond], (u64)__popcll(bb));
    atomicMin(&a.tot[kRdBadRange], r + (u64)__ffsll((unsigned long long)bb) - 1);
  }
  u64 before[1], all[1];
  block_scan<kReadThreads, 1>({cnt}, before, all);
  if (r < a.nranges) a.pref[r] = before[0];
  if (threadIdx.x == 0) a.blk[blockIdx.x] = all[0];
}

// the slots in front of range m
__device__ __forceinline__ u64 slots_before(const ReadArgs& a, u64 m) {
  return a.blk[m / kReadThreads] + a.pref[m];
}

// One lane per table slot, grid-stride.  The loads depend on each other (the
// range's prefix, the chunk's ends, its ID, the store's slot, the stored ID,
// the stored ends): the waves of the other slots hide them.
__global__ __launch_bounds__(kReadThreads) void read_emit_kernel(ReadArgs a) {
  const u64 total = a.tot[kRdSlots];
  if (total > a.cap) {  // (uniform over the grid: nothing is written)
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tot[kRdOverflow] = 1;
    return;
  }
  const u64 stride = (u64)gridDim.x * kReadThreads;
  for (u64 base = (u64)blockIdx.x * kReadThreads; base < total; base += stride) {
    const u64 k = base + threadIdx.x;
    bool piece = false, miss = false, wrong = false;
    u64 from_store = 0, from_null = 0, bad_range = kNone, bad_chunk = kNone;
    if (k < total) {
      // the last range whose slots begin at or below k: it has slots, k is one
      u64 l = 0, h = a.nranges;
      while (l < h) {
        const u64 m = l + ((h - l) >> 1);
        if (slots_before(a, m) > k) h = m;
        else l = m + 1;
      }
      const u64 r = l - 1;  // (l >= 1: range 0 begins at slot 0)
      const u64 i = (u64)a.first[r] + (k - slots_before(a, r));
      AsmSeg g;
      g.dst_off = a.ranges[3 * r + 2];
      g.bytes = 0;
      g.src = nullptr;
      if (i < a.n) {  // (always: the count kept first + count <= n)
        const u64 cs = i ? a.ends[i - 1] : a.start, ce = a.ends[i];
        const dsx_read::Piece p =
            dsx_read::piece_of(cs, ce, a.ranges[3 * r], a.ranges[3 * r + 1], a.ranges[3 * r + 2]);
        g.dst_off = p.dst_off;
        wrong = p.bad_ends;
        if (p.bytes) {
          piece = true;
          const u64 size = ce - cs;
          const Id32 key = load_id(a.ids, i);
          if (a.has_null && same_id(key, a.null_id)) {
            wrong = size != a.null_size;
            if (!wrong) g.bytes = p.bytes, from_null = p.bytes;
          } else {
            const uint32_t e = store_find(a.st, key);
            miss = e == kEmpty;
            if (!miss) {
              const u64 lo = e ? a.st.ends[e - 1] : 0, hi = a.st.ends[e];
              // (hi <= st.bytes in a store the library filled: no record points outside the arena)
              wrong = hi < lo || hi - lo != size || hi > a.st.bytes;
              if (!wrong) {
                g.bytes = p.bytes, from_store = p.bytes;
                g.src = a.st.arena + lo + p.chunk_off;
              }
            }
          }
        }
        if (miss || wrong) bad_range = r, bad_chunk = i;
      }
      a.segs[k] = g;
    }
    const u64 bp = __ballot(piece), bm = __ballot(miss), bw = __ballot(wrong);
    const u64 sb = wave_sum(from_store), nb = wave_sum(from_null);
    if (bm | bw) {  // (uniform over the wave)
      bad_range = wave_min(bad_range);
      bad_chunk = wave_min(bad_chunk);
    }
    if ((threadIdx.x & 63) == 0) {
      if (bp) atomicAdd(&a.tot[kRdPieces], (u64)__popcll(bp));
      if (sb) atomicAdd(&a.tot[kRdStoreBytes], sb);
      if (nb) atomicAdd(&a.tot[kRdNullBytes], nb);
      if (bm) atomicAdd(&a.tot[kRdMissing], (u64)__popcll(bm));
      if (bw) atomicAdd(&a.tot[kRdWrong], (u64)__popcll(bw));
      if (bm | bw) {
        atomicMin(&a.tot[kRdBadRange], bad_range);
        atomicMin(&a.tot[kRdBadChunk], bad_chunk);
      }
    }
  }
}

}  // namespace dsx

using namespace dsx;

namespace {

int range_error(dsx_ctx* c, uint64_t r, const char* what) {
  return invalid(c, "range " + std::to_string(r) + ": " + what);
}

bool ends_ascend(const uint64_t* ends, uint64_t start, uint64_t n) {
  uint64_t prev = start;
  for (uint64_t i = 0; i < n; ++i) {
    if (ends[i] < prev) return false;
    prev = ends[i];
  }
  return true;
}

}  // namespace

extern "C" int dsx_read_plan(const uint64_t* ends, uint64_t start, uint64_t n,
                             const dsx_range_t* ranges, uint64_t nranges, dsx_read_piece_t* pieces,
                             uint64_t cap, uint64_t* npieces) {
  if (!npieces) return DSX_E_INVAL;
  *npieces = 0;
  if ((n && !ends) || (nranges && !ranges) || (cap && !pieces)) return DSX_E_INVAL;
  if (n > kCallMaxN || nranges > kCallMaxN) return DSX_E_INVAL;
  if (!ends_ascend(ends, start, n)) return DSX_E_INVAL;
  uint64_t k = 0;
  for (uint64_t r = 0; r < nranges; ++r) {
    const dsx_range_t& g = ranges[r];
    const dsx_read::Span s = dsx_read::span_of(ends, start, n, g.off, g.len);
    if (s.beyond) return DSX_E_INVAL;
    for (uint64_t i = s.first; i < s.first + s.count; ++i) {
      const dsx_read::Piece p =
          dsx_read::piece_of(i ? ends[i - 1] : start, ends[i], g.off, g.len, g.dst_off);
      if (!p.bytes) continue;
      if (k < cap) {
        dsx_read_piece_t& o = pieces[k];
        o.chunk_off = p.chunk_off;
        o.dst_off = p.dst_off;
        o.bytes = p.bytes;
        o.range = (uint32_t)r;
        o.chunk = (uint32_t)i;
      }
      ++k;
    }
  }
  *npieces = k;
  return k > cap ? DSX_E_CAPACITY : DSX_OK;
}

extern "C" int dsx_read_ranges(dsx_ctx_t* c, const dsx_store_t* s, const void* ids,
                               const uint64_t* ends, uint64_t start, uint64_t n,
                               const uint8_t* null_id, uint64_t null_size, const dsx_range_t* ranges,
                               uint64_t nranges, void* d_out, uint64_t out_len,
                               dsx_read_totals_t* totals, uint32_t flags) {
  const uint32_t f_ids = DSX_IDS_DEVICE, f_ends = DSX_ENDS_DEVICE;
  if (!c) return DSX_E_INVAL;
  if (!s || !totals) return invalid(c, "the store or the totals are missing");
  DSX_FLUSH_BEHIND(c);
  *totals = dsx_read_totals_t{};
  totals->first_bad_range = totals->first_bad_chunk = 0xFFFFFFFFu;
  // ---- every check comes before any device work ----------------------------------
  if ((flags & ~(f_ids | f_ends)) != 0) return invalid(c, "unknown flag bit");
  if (!owns(c, s)) return foreign_store(c, DSX_E_STATE);
  if (s->broken) return broken_store(c);
  if (nranges > kCallMaxN) return invalid(c, "more ranges than a call takes (0xFFFFFFF0)");
  if (n > kCallMaxN) return invalid(c, "more chunks than a call takes (0xFFFFFFF0)");
  if ((n && (!ids || !ends)) || (nranges && !ranges) || (out_len && !d_out))
    return invalid(c, "the IDs, the chunk ends, the ranges or the output are missing");
  if (out_len > UINT64_MAX - (uintptr_t)d_out) return invalid(c, "the output wraps the address space");
  uint64_t prev_off = 0, prev_end = 0, bytes = 0, out_lo = 0, out_hi = 0;
  for (uint64_t r = 0; r < nranges; ++r) {
    const dsx_range_t& g = ranges[r];
    if (g.len > out_len || g.dst_off > out_len - g.len)
      return range_error(c, r, "dst_off + len is beyond the output");
    if (g.dst_off < prev_off) return range_error(c, r, "dst_off is below the one before it");
    if (g.dst_off < prev_end)
      return range_error(c, r, "its destination window overlaps the one before it");
    prev_off = g.dst_off;
    prev_end = g.dst_off + g.len;
    if (g.len) {
      if (!bytes) out_lo = g.dst_off;
      out_hi = prev_end;
    }
    bytes += g.len;
  }
  if (overlaps(d_out, out_len, s->arena.p, s->arena_bytes))
    return invalid(c, "the output overlaps the store's arena");
  // the table's first size: exact with host ends, else a guess the emit corrects
  uint64_t slots = std::min<uint64_t>(bytes, 2 * nranges + 1024);
  if (!(flags & f_ends)) {
    if (!ends_ascend(ends, start, n))
      return invalid(c, "chunk ends must be non-decreasing and start <= ends[0]");
    slots = 0;
    for (uint64_t r = 0; r < nranges; ++r) {
      slots += dsx_read::span_of(ends, start, n, ranges[r].off, ranges[r].len).count;
      if (slots > kCallMaxN)
        return range_error(c, r, "more (range, chunk) pairs than a call takes (0xFFFFFFF0)");
    }
  }
  totals->ranges = nranges;
  totals->bytes = bytes;
  if (nranges == 0) return DSX_OK;

  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;
  // ---- stage ---------------------------------------------------------------------
  static_assert(sizeof(dsx_range_t) == 24, "three words a range (StoreScratch::rd_ranges)");
  ReadArgs a{};
  a.ids = (const uint8_t*)ids;  // (an index without chunks: nothing is staged, nothing reads them)
  a.ends = ends;
  int rc = n ? stage_ids(c, ids, n, (flags & f_ids) != 0, &a.ids) : DSX_OK;
  if (!rc && n) rc = stage_ends(c, ends, n, (flags & f_ends) != 0, &a.ends);
  if (rc) return rc;
  const uint64_t nblk = (nranges + kReadThreads - 1) / kReadThreads;
  HIPCHK(c, grow(c, w.rd_ranges, 3 * nranges));
  HIPCHK(c, grow(c, w.rd_pref, nranges));
  HIPCHK(c, grow(c, w.rd_first, nranges));
  HIPCHK(c, grow(c, w.rd_blk, nblk));
  HIPCHK(c, grow(c, w.rd_tot, kRdCounters));
  HIPCHK(c, grow(c, w.rd_segs, 3 * slots));
  HIPCHK(c, hipMemcpyAsync(w.rd_ranges.p, ranges, nranges * sizeof(dsx_range_t),
                           hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(w.rd_tot.p, 0, kRdCounters * sizeof(u64), st));
  HIPCHK(c, hipMemsetAsync(w.rd_tot.p + kRdBadRange, 0xFF, 2 * sizeof(u64), st));  // none

  a.ranges = w.rd_ranges.p;
  a.nranges = nranges;
  a.start = start;
  a.n = n;
  if (null_id) {
    memcpy(&a.null_id, null_id, 32);
    a.has_null = 1;
    a.null_size = null_size;
  }
  a.st = view_of(s);
  a.pref = w.rd_pref.p;
  a.first = w.rd_first.p;
  a.blk = w.rd_blk.p;
  a.nblk = nblk;
  a.tot = w.rd_tot.p;
  // ---- count, scan, emit -----------------------------------------------------------
  hipLaunchKernelGGL(read_count_kernel, dim3((uint32_t)nblk), dim3(kReadThreads), 0, st, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(block_array_scan_kernel<1>, dim3(1), dim3(kArrayScanThreads), 0, st, w.rd_blk.p,
                     (u64)nblk, w.rd_tot.p + kRdSlots);
  HIPCHK(c, hipGetLastError());
  // The emit's grid: enough workgroups for the slots the table can hold, at most
  // 8 a CU; the lanes stride over the rest.
  u64 tot[kRdCounters] = {};
  for (int pass = 0; pass < 2; ++pass) {
    a.segs = reinterpret_cast<AsmSeg*>(w.rd_segs.p);
    a.cap = w.rd_segs.n / 3;
    const uint64_t want = (a.cap + kReadThreads - 1) / kReadThreads;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, 8ull * c->ncu));
    hipLaunchKernelGGL(read_emit_kernel, dim3(grid), dim3(kReadThreads), 0, st, a);
    HIPCHK(c, hipGetLastError());
    // ---- the one wait before any byte is written -----------------------------------
    HIPCHK(c, hipMemcpyAsync(tot, w.rd_tot.p, sizeof tot, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (!tot[kRdOverflow]) break;
    if (pass == 1) {
      c->err = "the gather table did not grow";
      return DSX_E_INTERNAL;
    }
    if (tot[kRdSlots] > kCallMaxN)
      return invalid(c, "more (range, chunk) pairs than a call takes (0xFFFFFFF0)");
    HIPCHK(c, grow(c, w.rd_segs, 3 * tot[kRdSlots]));
    HIPCHK(c, hipMemsetAsync(w.rd_tot.p + kRdOverflow, 0, sizeof(u64), st));
  }
  totals->pieces = tot[kRdPieces];
  totals->store_bytes = tot[kRdStoreBytes];
  totals->null_bytes = tot[kRdNullBytes];
  totals->missing = tot[kRdMissing];
  totals->wrong_size = tot[kRdWrong];
  totals->beyond = tot[kRdBeyond];
  totals->first_bad_range = tot[kRdBadRange] == kNone ? 0xFFFFFFFFu : (uint32_t)tot[kRdBadRange];
  totals->first_bad_chunk = tot[kRdBadChunk] == kNone ? 0xFFFFFFFFu : (uint32_t)tot[kRdBadChunk];
  if (tot[kRdMissing] || tot[kRdWrong] || tot[kRdBeyond]) return DSX_OK;  // (the counts are the answer)
  // ---- gather ------------------------------------------------------------------------
  rc = assemble_launch(c, a.segs, tot[kRdSlots], d_out, out_len, out_lo, out_hi, false);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(st));
  return DSX_OK;
}
