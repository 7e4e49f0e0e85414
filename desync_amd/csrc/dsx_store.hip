// dsx_store.hip -- a chunk store in HBM (store.go:21-33, local.go,
// chunkstorage.go): a deduplicating, tightly packed arena of chunk bytes keyed
// by chunk ID, filled from a resident blob without a host round trip per
// chunk, read in place by dsx_assemble and, range by range, by dsx_read_ranges
// (dsx_read.hip), and pruned in place (PruneStore.Prune, local.go:163-202).  The counterpart of a LocalStore with Uncompressed: true
// (store.go:98-99).
//
// Layout (dsx_store.h): entry e is the e-th chunk appended that no prune has
// removed; ids[32 e] is its ID, arena[ends[e-1], ends[e]) its bytes.  The ID
// table is dsx_idset.hip's, with entry numbers for positions: between two
// prunes a full slot never changes.  Capacity is fixed at creation, so the
// arena's address is stable and dsx_assemble can be handed it as the store
// buffer.
//
// A put is a fixed sequence of launches on the context's stream:
//   select  the call's own table (idset_insert_kernel), then one lane per
//           chunk: new[i] = first occurrence in this call and not in the
//           store; the same kernel validates the chunk ends, reduces the
//           totals and leaves {new chunks, new bytes} per workgroup;
//   scan    one workgroup turns those pairs into exclusive prefix sums;
//   (the host reads the totals and the error word, and accepts the capacity)
//   append  each new chunk takes entry chunks + rank and arena offset bytes +
//           prefix (its rank and its byte offset inside the workgroup by
//           block_scan, dsx_blockscan.h), writes its ID, its end and a gather
//           record, and claims a table slot;
//   copy    assemble_kernel over the gather records into arena[used, used +
//           stored_bytes): tiles are cut over the destination.
// The IDs appended in one call differ from each other and from every ID the
// store holds (that is what select selected).  The insert therefore claims
// the first empty slot on its probe sequence and compares no ID
// (idset_claim_empty, dsx_idset_dev.h, has why).
//
// A prune is the put turned around (DESIGN.md 4.7 has the safety argument):
//   mark     the call's own table over ids[], then one lane per entry: keep[e],
//            the totals, {kept entries, kept bytes} per workgroup;
//   scan     the put's;
//   (the host reads the totals; nothing removed: the call returns)
//   compact  each survivor's new entry number and arena offset, as the append
//            finds them; its ID, its new end and a gather record go to scratch;
//   move     window by window over the destination [first removed byte, new
//            used): assemble_kernel gathers a window's bytes from their old
//            places into a bounce buffer, a copy writes the buffer over the
//            window.  Every byte moves left or stays, so what a window's
//            write-back destroys has been read by this or an earlier window,
//            and what a later window needs lies behind it;
//   rebuild  the new IDs and ends are copied over the store's, the table is
//            cleared and every survivor claims a slot as the append does.
//
// A copy between two stores (Copy, copy.go:9-58) is the put with a second store
// for the blob:
//   select  the call's own table, then one lane per ID: copy[i] = first
//           occurrence in this call, not in dst, in src (dst is asked first,
//           copy.go:27-33); the source entry's number and its size from src's
//           ends; the totals, the lowest position of an ID neither store holds,
//           and {chunks, bytes} per workgroup.  DSX_COPY_ALL reads src's IDs
//           where they lie: they are distinct and lane i's entry is i, so it
//           builds no table and probes only dst;
//   scan    the put's;
//   (the host reads the totals: an ID missing from both stores, or a copy that
//   does not fit, ends the call here, before dst is written anywhere)
//   append  the put's, with the gather record pointing into src's arena;
//   copy    assemble_kernel into dst.arena[used, used + copied_bytes).
// The appended IDs again differ from each other and from all of dst's, so the
// claim compares none.  src is only read.  A store grows by a copy of all its
// entries into a larger one.
//
// An evict (dsx_store_evict, of a store that tracks use: one stamp per entry)
// is a prune whose keep mask the device chooses (Eviction):
//   pins     the call's own table over the pin list, pinned[e], the sums of the rest;
//   descent  per stamp byte, from the clock's highest down: a histogram of 256
//            {entries, bytes} buckets over the unpinned entries under the bytes
//            chosen so far, then one workgroup picks the bucket in which the
//            least recently used prefix that makes the room ends
//            (dsx_evict_geom.h); no host wait between the passes;
//   class    {entries, bytes} of the cutoff stamp's class per workgroup, scanned;
//   keep     keep[e] = pinned, or newer than the cutoff, or of its class behind
//            a class prefix that already meets the needs; what mark leaves;
//   (the host reads the totals; from here on it is the prune's compact, move
//   and rebuild, one function for both, with the stamps carried along)
//
// Out of scope: compression and encryption converters; persistence
// (dsx_store_entries plus the arena are enough for a caller to save and reload
// one); use from a second context or GPU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dsx_callargs.h"
#include "dsx_engine.h"
#include "dsx_evict_geom.h"
#include "dsx_idset_dev.h"

namespace dsx {

constexpr int kStoreThreads = 256;

struct PutArgs {
  const uint8_t* ids;  // the call's IDs
  // a put's blob: its chunk ends, where chunk 0 starts, its length
  const uint64_t* ends;
  u64 start, n, len;
  const uint8_t* blob;
  const uint32_t* slots;  // the call's own table (built by the launch before)
  u64 mask, salt;
  StoreView dst;   // the store the chunks go to
  uint8_t* flag;   // new[i]
  u64* blk;        // {chunks, bytes} per workgroup
  u64* tot;        // [kStoreCounters]
  AsmSeg* segs;    // [n_new], written by the append
  u64 n_new;       // the accepted total: the append's ranks stay below it
  StoreView src;   // a copy between stores: the store they come from, in place of the blob
  u64 all;         // DSX_COPY_ALL: ids is src.ids, ID i is entry i, no table of the call's, src's not probed
  uint32_t* srce;  // [n] the source entry of ID i (written where flag[i] is set)
};

// One lane per chunk.  A chunk whose end lies below its start or beyond the
// blob sets the error word (the host then stops before the append).
__global__ __launch_bounds__(kStoreThreads) void store_select_kernel(PutArgs a) {
  const u64 i = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool is_new = false, present = false, bad = false;
  u64 size = 0;
  if (i < a.n) {
    const u64 e = a.ends[i], prev = i ? a.ends[i - 1] : a.start;
    bad = e < prev || e > a.len;
    const Id32 me = load_id(a.ids, i);
    if (idset_find(a.ids, a.n, a.slots, a.mask, a.salt, me) == (uint32_t)i) {
      present = store_find(a.dst, me) != kEmpty;
      is_new = !present;
    }
    if (is_new && !bad) size = e - prev;
    a.flag[i] = is_new ? 1 : 0;
  }
  const u64 bn = __ballot(is_new), bp = __ballot(present), bb = __ballot(bad);
  const u64 bytes = wave_sum(size);
  if ((threadIdx.x & 63) == 0) {
    if (bn) atomicAdd(&a.tot[0], (u64)__popcll(bn));
    if (bytes) atomicAdd(&a.tot[1], bytes);
    if (bp) atomicAdd(&a.tot[2], (u64)__popcll(bp));
    if (bb) atomicOr(&a.tot[3], 1ull);
  }
  block_totals_to<kStoreThreads, 2>({(u64)__popcll(bn), bytes}, a.blk);
}

// The bytes of entry e of a copy's source, [*lo, *lo + size): 0 for an entry
// whose ends are not inside the used arena (never, in a store the library
// filled), so that no gather record points outside it.
__device__ __forceinline__ u64 copy_extent(const StoreView& src, uint32_t e, u64* lo) {
  const u64 prev = e ? src.ends[e - 1] : 0, end = src.ends[e];
  *lo = prev;
  return prev <= end && end <= src.bytes ? end - prev : 0;
}

// One lane per ID of a copy between stores.  tot[4] starts at UINT64_MAX.
__global__ __launch_bounds__(kStoreThreads) void store_copy_select_kernel(PutArgs a) {
  const u64 i = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool is_new = false, present = false, missing = false;
  u64 size = 0;
  if (i < a.n) {
    const Id32 me = load_id(a.ids, i);
    if (a.all || idset_find(a.ids, a.n, a.slots, a.mask, a.salt, me) == (uint32_t)i) {
      present = store_find(a.dst, me) != kEmpty;
      if (!present) {
        const uint32_t e = a.all ? (uint32_t)i : store_find(a.src, me);
        missing = e == kEmpty;
        if (!missing) {
          u64 lo;
          is_new = true;
          size = copy_extent(a.src, e, &lo);
          a.srce[i] = e;
        }
      }
    }
    a.flag[i] = is_new ? 1 : 0;
  }
  const u64 bn = __ballot(is_new), bp = __ballot(present), bm = __ballot(missing);
  const u64 bytes = wave_sum(size);
  if ((threadIdx.x & 63) == 0) {
    if (bn) atomicAdd(&a.tot[0], (u64)__popcll(bn));
    if (bytes) atomicAdd(&a.tot[1], bytes);
    if (bp) atomicAdd(&a.tot[2], (u64)__popcll(bp));
    if (bm) {
      atomicAdd(&a.tot[3], (u64)__popcll(bm));
      atomicMin(&a.tot[4], i + (u64)__ffsll((unsigned long long)bm) - 1);  // (lane 0's i: the wave's first)
    }
  }
  block_totals_to<kStoreThreads, 2>({(u64)__popcll(bn), bytes}, a.blk);
}

// Entry e of ids[] / ends[]: its ID, its end and its gather record (size bytes
// from src to arena offset off).
__device__ __forceinline__ void write_entry(uint8_t* ids, uint64_t* ends, u64 e, const Id32& me, u64 off,
                                            u64 size, const uint8_t* src, AsmSeg* seg) {
  uint4* dst = reinterpret_cast<uint4*>(ids + 32 * e);
  dst[0] = me.lo;
  dst[1] = me.hi;
  ends[e] = off + size;
  AsmSeg g;
  g.dst_off = off;
  g.bytes = size;
  g.src = src;
  *seg = g;
}

// One lane per chunk, the grid of store_select_kernel.  Runs only after the
// host has accepted the capacity: entry numbers stay below max_chunks and the
// table keeps an empty slot (load factor <= 0.5).  COPY: the chunk is entry
// srce[i] of the source store (PutArgs), not chunk i of the blob.
template <bool COPY>
__global__ __launch_bounds__(kStoreThreads) void store_append_kernel(PutArgs a) {
  const u64 i = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool is_new = false;
  u64 size = 0, prev = 0;
  if (i < a.n && a.flag[i]) {
    is_new = true;
    if constexpr (COPY) {
      size = copy_extent(a.src, a.srce[i], &prev);  // (as select sized it: never reads past the used arena)
    } else {
      const u64 e = a.ends[i];
      prev = i ? a.ends[i - 1] : a.start;
      if (prev <= e && e <= a.len) size = e - prev;  // (select checked it: never reads past the blob)
    }
  }
  u64 before[2], all[2];
  block_scan<kStoreThreads, 2>({is_new ? 1ull : 0ull, size}, before, all);
  if (!is_new) return;
  const u64 rank = a.blk[2 * (u64)blockIdx.x] + before[0];
  if (rank >= a.n_new) return;  // (never: the ranks are the scan of the flags the total counted)
  const u64 e = a.dst.n + rank;
  const u64 off = a.dst.bytes + a.blk[2 * (u64)blockIdx.x + 1] + before[1];
  const Id32 me = load_id(a.ids, i);
  write_entry(a.dst.ids, a.dst.ends, e, me, off, size, (COPY ? a.src.arena : a.blob) + prev, &a.segs[rank]);
  idset_claim_empty(a.dst.slots, a.dst.mask, a.dst.salt, me, (uint32_t)e);
}

// One lane per question: ids[idx ? idx[i] : i] looked up in the store.
__global__ __launch_bounds__(kStoreThreads) void store_lookup_kernel(const uint8_t* ids,
                                                                     const uint32_t* idx, u64 n,
                                                                     StoreView st, uint64_t* offs,
                                                                     uint64_t* sizes, u64* missing) {
  const u64 i = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool miss = false;
  if (i < n) {
    const Id32 key = load_id(ids, idx ? idx[i] : i);
    const uint32_t e = store_find(st, key);
    miss = e == kEmpty;
    const u64 lo = miss ? UINT64_MAX : (e ? st.ends[e - 1] : 0);
    if (offs) offs[i] = lo;
    if (sizes) sizes[i] = miss ? 0 : st.ends[e] - lo;
  }
  const u64 bm = __ballot(miss);
  if ((threadIdx.x & 63) == 0 && bm) atomicAdd(missing, (u64)__popcll(bm));
}

// flag[e] = the computed ID of entry e differs from the stored one
__global__ __launch_bounds__(kStoreThreads) void store_compare_kernel(const uint8_t* got,
                                                                      const uint8_t* want, u64 n,
                                                                      uint8_t* flag, u64* n_bad) {
  const u64 i = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool bad = false;
  if (i < n) {
    bad = !same_id(load_id(got, i), load_id(want, i));
    flag[i] = bad ? 1 : 0;
  }
  const u64 bb = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && bb) atomicAdd(n_bad, (u64)__popcll(bb));
}

struct PruneArgs {
  const uint8_t* ids;     // the call's IDs ...
  const uint32_t* slots;  // ... and the table over them
  u64 n, mask, salt;
  u64 invert;             // DSX_PRUNE_REMOVE: ids[] names the entries to drop
  StoreView st;           // the store before the prune (only read: the rebuild is the host's copies)
  uint8_t* flag;       // keep[e]
  u64* blk;            // {kept entries, kept bytes} per workgroup
  u64* tot;            // [kStoreCounters]
  uint8_t* new_ids;    // [kept], written by the compaction
  uint64_t* new_ends;  // [kept]
  AsmSeg* segs;        // [kept]
  u64 n_keep;          // the total the host read: the compaction's ranks stay below it
  const uint64_t* stamps;  // a tracked store's stamps, else null ...
  uint64_t* new_stamps;    // ... and [kept], the survivors' (null with stamps)
  uint8_t* ev_ids;     // an evict that reports its victims: [n_ev] their IDs in entry order, else null
  u64 n_ev;
};

// One lane per entry: keep[e] = the entry's ID is among the call's (is not,
// with invert).  tot[2] takes UINT64_MAX - the lowest offset of a removed entry
// that has bytes: in front of that offset no byte moves.
__global__ __launch_bounds__(kStoreThreads) void store_mark_kernel(PruneArgs a) {
  const u64 e = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool keep = false;
  u64 size = 0, gone_at = 0;
  if (e < a.st.n) {
    const bool named = idset_find(a.ids, a.n, a.slots, a.mask, a.salt, load_id(a.st.ids, e)) != kEmpty;
    keep = named != (a.invert != 0);
    const u64 lo = e ? a.st.ends[e - 1] : 0, hi = a.st.ends[e];
    if (keep) size = hi - lo;
    else if (hi > lo) gone_at = UINT64_MAX - lo;
    a.flag[e] = keep ? 1 : 0;
  }
  const u64 bk = __ballot(keep);
  const u64 bytes = wave_sum(size);
  gone_at = wave_max(gone_at);
  if ((threadIdx.x & 63) == 0) {
    if (bk) atomicAdd(&a.tot[0], (u64)__popcll(bk));
    if (bytes) atomicAdd(&a.tot[1], bytes);
    if (gone_at) atomicMax(&a.tot[2], gone_at);
  }
  block_totals_to<kStoreThreads, 2>({(u64)__popcll(bk), bytes}, a.blk);
}

// One lane per entry, the grid of store_mark_kernel, after the scan: survivor e
// becomes entry `rank` at arena offset `off`.  The new IDs and ends go to
// scratch (written in place they would overwrite entries another lane of this
// launch still has to read); every survivor leaves a gather record, those in
// front of the first removed byte with src == the place they already have.
__global__ __launch_bounds__(kStoreThreads) void store_compact_kernel(PruneArgs a) {
  const u64 e = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool keep = false;
  u64 size = 0, old = 0;
  if (e < a.st.n && a.flag[e]) {
    keep = true;
    old = e ? a.st.ends[e - 1] : 0;
    size = a.st.ends[e] - old;
  }
  u64 before[2], all[2];
  block_scan<kStoreThreads, 2>({keep ? 1ull : 0ull, size}, before, all);
  const u64 rank = a.blk[2 * (u64)blockIdx.x] + before[0];
  const u64 off = a.blk[2 * (u64)blockIdx.x + 1] + before[1];
  const bool moved = keep && off != old;
  if (keep && rank < a.n_keep) {  // (always: the ranks are the scan of the flags the total counted)
    write_entry(a.new_ids, a.new_ends, rank, load_id(a.st.ids, e), off, size, a.st.arena + old,
                &a.segs[rank]);
    if (a.new_stamps) a.new_stamps[rank] = a.stamps[e];
  }
  // a victim's place among the victims: its entry number less the survivors in front of it
  if (a.ev_ids && e < a.st.n && !keep && e - rank < a.n_ev) {
    const Id32 me = load_id(a.st.ids, e);
    uint4* dst = reinterpret_cast<uint4*>(a.ev_ids + 32 * (e - rank));
    dst[0] = me.lo;
    dst[1] = me.hi;
  }
  const u64 bm = __ballot(moved);
  const u64 mb = wave_sum(moved ? size : 0);
  if ((threadIdx.x & 63) == 0) {
    if (bm) atomicAdd(&a.tot[4], (u64)__popcll(bm));
    if (mb) atomicAdd(&a.tot[5], mb);
  }
}

// One lane per entry of the compacted store: the put's claim into the cleared
// table (the stored IDs differ from each other).
__global__ __launch_bounds__(kStoreThreads) void store_reclaim_kernel(const uint8_t* st_ids, u64 st_n,
                                                                      uint32_t* st_slots, u64 st_mask,
                                                                      u64 st_salt) {
  const u64 e = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  if (e < st_n) idset_claim_empty(st_slots, st_mask, st_salt, load_id(st_ids, e), (uint32_t)e);
}

// ---- use tracking and eviction -------------------------------------------------------
// One lane per ID: the entry that holds it takes the stamp.  Lanes that name
// one entry write one value to one word.  missing (may be null) counts the
// positions the store does not hold.  store_find answers below st.n only.
__global__ __launch_bounds__(kStoreThreads) void store_touch_kernel(const uint8_t* ids, u64 n,
                                                                    StoreView st, uint64_t* stamps,
                                                                    u64 stamp, u64* missing) {
  const u64 i = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool miss = false;
  if (i < n) {
    const uint32_t e = store_find(st, load_id(ids, i));
    miss = e == kEmpty;
    if (!miss) stamps[e] = stamp;
  }
  if (missing) {
    const u64 bm = __ballot(miss);
    if ((threadIdx.x & 63) == 0 && bm) atomicAdd(missing, (u64)__popcll(bm));
  }
}

// One lane per ID of a copy: the source entry of a copied ID takes the stamp.
__global__ __launch_bounds__(kStoreThreads) void store_touch_source_kernel(const uint8_t* flag,
                                                                           const uint32_t* srce, u64 n,
                                                                           uint64_t* stamps, u64 src_n,
                                                                           u64 stamp) {
  const u64 i = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  if (i < n && flag[i] && srce[i] < src_n) stamps[srce[i]] = stamp;
}

struct EvictArgs {
  const uint8_t* pin_ids;     // the pin list ...
  const uint32_t* pin_slots;  // ... and the table over it
  u64 n_pin, pin_mask, pin_salt;
  StoreView st;
  const uint64_t* stamps;  // [st.n]
  uint8_t* pinned;         // [st.n]
  u64* sel;                // [kEvictSel]
  u64* hist;               // this pass's 256 {entries, bytes} pairs
  u64* cblk;               // the boundary class's {entries, bytes} per workgroup
  uint8_t* flag;           // keep[e], and what store_mark_kernel leaves beside it:
  u64* blk;
  u64* tot;
  u64 need_chunks, need_bytes;  // the call's, less the room the store has
  int level, first;        // the stamp byte of this pass; first: the needs are the call's, not sel's
};

__device__ __forceinline__ u64 entry_size(const StoreView& st, u64 e) {
  return st.ends[e] - (e ? st.ends[e - 1] : 0);
}

// One lane per entry: pinned[e] = the entry's ID is in the pin list; the sums of
// the others.
__global__ __launch_bounds__(kStoreThreads) void evict_pin_kernel(EvictArgs a) {
  const u64 e = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool pin = false, free_ = false;
  u64 size = 0;
  if (e < a.st.n) {
    pin = idset_find(a.pin_ids, a.n_pin, a.pin_slots, a.pin_mask, a.pin_salt, load_id(a.st.ids, e)) != kEmpty;
    free_ = !pin;
    if (free_) size = entry_size(a.st, e);
    a.pinned[e] = pin ? 1 : 0;
  }
  const u64 bp = __ballot(pin), bf = __ballot(free_);
  const u64 bytes = wave_sum(size);
  if ((threadIdx.x & 63) == 0) {
    if (bf) atomicAdd(&a.sel[kSelEvictable], (u64)__popcll(bf));
    if (bytes) atomicAdd(&a.sel[kSelEvictableBytes], bytes);
    if (bp) atomicAdd(&a.sel[kSelPinned], (u64)__popcll(bp));
  }
}

// One pass of the descent, one lane per entry: an unpinned entry whose stamp
// bytes above `level` are the ones chosen so far adds {1, size} to the bucket
// of its byte `level`, in LDS; then one global add per non-empty sum.  A wave
// whose entries all fall into one bucket (every pass above the byte in which
// the stamps differ, and every pass of a store with one stamp) adds its two
// sums once, from lane 0; a wave with several buckets adds per lane.  Integer
// adds: the histogram does not depend on their order, nor on which way a wave went.
__global__ __launch_bounds__(kStoreThreads) void evict_hist_kernel(EvictArgs a) {
  __shared__ u64 s_hist[2 * dsx_evict::kBuckets];
  if (a.sel[kSelFailed]) return;  // (the whole grid: nothing below reads the histogram)
  for (int k = threadIdx.x; k < 2 * dsx_evict::kBuckets; k += kStoreThreads) s_hist[k] = 0;
  __syncthreads();
  const u64 e = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  bool mine = false;
  uint32_t b = 0;
  u64 size = 0;
  if (e < a.st.n && !a.pinned[e]) {
    const u64 s = a.stamps[e];
    const u64 above = a.level >= 7 ? 0 : s >> (8 * (a.level + 1));
    if (above == a.sel[kSelPrefix]) {
      mine = true;
      b = (uint32_t)(s >> (8 * a.level)) & 255u;
      size = entry_size(a.st, e);
    }
  }
  const u64 bm = __ballot(mine);
  if (bm) {  // (wave-uniform)
    const uint32_t first = __shfl(b, __ffsll((unsigned long long)bm) - 1, 64);
    if (__ballot(mine && b == first) == bm) {
      const u64 bytes = wave_sum(size);  // (size is 0 in the lanes without an entry)
      if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_hist[2 * first], (u64)__popcll(bm));
        if (bytes) atomicAdd(&s_hist[2 * first + 1], bytes);
      }
    } else if (mine) {
      atomicAdd(&s_hist[2 * b], 1ull);
      if (size) atomicAdd(&s_hist[2 * b + 1], size);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * dsx_evict::kBuckets; k += kStoreThreads)
    if (s_hist[k]) atomicAdd(&a.hist[k], s_hist[k]);
}

// One workgroup: the bucket the prefix ends in (dsx_evict_geom.h), the chosen
// byte appended to the prefix and the needs lowered by the sums below it.
__global__ __launch_bounds__(kStoreThreads) void evict_choose_kernel(EvictArgs a) {
  __shared__ dsx_evict::Pair s_pair[dsx_evict::kBuckets];
  for (int k = threadIdx.x; k < dsx_evict::kBuckets; k += kStoreThreads) {
    s_pair[k].count = a.hist[2 * k];
    s_pair[k].bytes = a.hist[2 * k + 1];
  }
  __syncthreads();
  if (threadIdx.x != 0 || a.sel[kSelFailed]) return;
  const u64 nc = a.first ? a.need_chunks : a.sel[kSelNeedChunks];
  const u64 nb = a.first ? a.need_bytes : a.sel[kSelNeedBytes];
  const dsx_evict::Choice c = dsx_evict::choose(s_pair, nc, nb);
  if (c.bucket < 0) {
    a.sel[kSelFailed] = 1;
    return;
  }
  a.sel[kSelPrefix] = (a.sel[kSelPrefix] << 8) | (u64)c.bucket;
  a.sel[kSelNeedChunks] = c.need_chunks;
  a.sel[kSelNeedBytes] = c.need_bytes;
}

// unpinned and stamped with the cutoff T: the class the prefix ends in
__device__ __forceinline__ bool in_class(const EvictArgs& a, u64 e) {
  return e < a.st.n && !a.sel[kSelFailed] && !a.pinned[e] && a.stamps[e] == a.sel[kSelPrefix];
}

// One lane per entry: {entries, bytes} of the boundary class per workgroup.
__global__ __launch_bounds__(kStoreThreads) void evict_class_kernel(EvictArgs a) {
  const u64 e = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  const bool mine = in_class(a, e);
  const u64 bc = __ballot(mine);
  const u64 bytes = wave_sum(mine ? entry_size(a.st, e) : 0);
  block_totals_to<kStoreThreads, 2>({(u64)__popcll(bc), bytes}, a.cblk);
}

// One lane per entry, after the scan of cblk: keep[e] = pinned, or stamped above
// T, or of the class T behind a class prefix that already meets the needs.
// Leaves what store_mark_kernel leaves.
__global__ __launch_bounds__(kStoreThreads) void evict_keep_kernel(EvictArgs a) {
  const u64 e = (u64)blockIdx.x * kStoreThreads + threadIdx.x;
  const bool mine = in_class(a, e);
  const u64 my_size = e < a.st.n ? entry_size(a.st, e) : 0;
  u64 before[2], all[2];
  block_scan<kStoreThreads, 2>({mine ? 1ull : 0ull, mine ? my_size : 0ull}, before, all);
  bool keep = false;
  u64 size = 0, gone_at = 0;
  if (e < a.st.n) {
    if (mine) {
      keep = a.cblk[2 * (u64)blockIdx.x] + before[0] >= a.sel[kSelNeedChunks] &&
             a.cblk[2 * (u64)blockIdx.x + 1] + before[1] >= a.sel[kSelNeedBytes];
    } else {
      keep = a.sel[kSelFailed] || a.pinned[e] || a.stamps[e] > a.sel[kSelPrefix];
    }
    if (keep) size = my_size;
    else if (my_size) gone_at = UINT64_MAX - (e ? a.st.ends[e - 1] : 0);
    a.flag[e] = keep ? 1 : 0;
  }
  const u64 bk = __ballot(keep);
  const u64 bytes = wave_sum(size);
  gone_at = wave_max(gone_at);
  if ((threadIdx.x & 63) == 0) {
    if (bk) atomicAdd(&a.tot[0], (u64)__popcll(bk));
    if (bytes) atomicAdd(&a.tot[1], bytes);
    if (gone_at) atomicMax(&a.tot[2], gone_at);
  }
  block_totals_to<kStoreThreads, 2>({(u64)__popcll(bk), bytes}, a.blk);
}

}  // namespace dsx

using namespace dsx;

namespace {

constexpr uint64_t kPruneWindow = 256ull << 20;  // dsx_store_prune's window == 0 (DESIGN.md 4.7 has the sweep)

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kStoreThreads - 1) / kStoreThreads); }

void free_store(dsx_store* s) {
  s->ids.release();
  s->ends.release();
  s->slots.release();
  s->arena.release();
  s->stamps.release();
  delete s;
}

// The front half of a put, a copy and a prune, up to the one host wait of the
// call before anything of a store is written: the flags, the workgroups' pairs
// and the counters grown, the counters cleared, the caller's select (which sets
// its arguments' flag, blk and tot from the scratch, presets a counter that
// does not start at 0, and launches its kernel over `blocks` workgroups), the
// array scan, the counters read back into tot[], and the wait.  distinct (a
// prune's): the distinct IDs the call's table counted, read in the same wait.
template <class Select>
int select_scan_wait(dsx_ctx* c, uint64_t items, Select&& select, u64 (&tot)[kStoreCounters],
                     u64* distinct = nullptr) {
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;
  const uint32_t blocks = blocks_of(items);
  HIPCHK(c, grow(c, w.flag, items));
  HIPCHK(c, grow(c, w.blk, 2 * (uint64_t)blocks));
  HIPCHK(c, grow(c, w.tot, kStoreCounters));
  HIPCHK(c, hipMemsetAsync(w.tot.p, 0, kStoreCounters * sizeof(u64), st));
  if (blocks) {
    const int rc = select(blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(block_array_scan_kernel<2>, dim3(1), dim3(kArrayScanThreads), 0, st, w.blk.p,
                       (u64)blocks, (u64*)nullptr);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(tot, w.tot.p, sizeof tot, hipMemcpyDeviceToHost, st));
  if (distinct)
    HIPCHK(c, hipMemcpyAsync(distinct, c->idset.tot.p, sizeof *distinct, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return DSX_OK;
}

// The back half of a prune and of an evict, behind the wait that read the kept
// count and bytes and UINT64_MAX - the first removed offset into tot[]
// (a.flag, a.blk and a.st are set, something is removed): the compaction of
// the metadata into scratch, the windowed move of the arena, the write-back of
// IDs, ends and a tracked store's stamps, the table rebuild, the last wait.
// tot[4], tot[5] end as the moved entries and bytes.  A failure past the first
// write leaves the store broken.  evicted (host, may be null): the IDs of the
// entries that go, the first a.n_ev in entry order, read in the same wait.
// dry: the scratch is filled and read, the store is not touched.
int compact_tail(dsx_ctx* c, dsx_store* s, PruneArgs& a, uint64_t kept, uint64_t kept_bytes,
                 u64 (&tot)[kStoreCounters], uint64_t window, bool dry, uint8_t* evicted) {
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;
  const uint64_t T = DSX_ASSEMBLE_TILE;
  const uint32_t blocks = blocks_of(s->chunks);
  // ---- compact the metadata (into scratch) ---------------------------------------
  uint64_t win = std::min<uint64_t>(window ? window : kPruneWindow, 1ull << 62);
  win = (win + T - 1) / T * T;
  win = std::min<uint64_t>(win, (s->arena_bytes + 15 + T) / T * T);  // (an arena's tiles: it never needs more)
  const uint64_t first_off = tot[2] ? UINT64_MAX - tot[2] : kept_bytes;  // in front of it nothing moves
  const bool moves = first_off < kept_bytes;
  if (!evicted) a.n_ev = 0;
  if (kept || a.n_ev) {
    // (no headroom: these are sized by the store and the window, not by a call that may grow)
    HIPCHK(c, grow(c, w.pids, kept * 32, false));
    HIPCHK(c, grow(c, w.pends, kept, false));
    HIPCHK(c, grow(c, w.segs, 3 * kept));
    if (moves && !dry) HIPCHK(c, grow(c, w.bounce, win, false));
    a.new_ids = w.pids.p;
    a.new_ends = (uint64_t*)w.pends.p;
    a.segs = reinterpret_cast<AsmSeg*>(w.segs.p);
    a.n_keep = kept;
    if (s->tracked) {
      HIPCHK(c, grow(c, w.pstamps, kept, false));
      a.stamps = s->stamps.p;
      a.new_stamps = (uint64_t*)w.pstamps.p;
    }
    if (a.n_ev) {
      HIPCHK(c, grow(c, w.ev_ids, a.n_ev * 32));
      a.ev_ids = w.ev_ids.p;
    }
    hipLaunchKernelGGL(store_compact_kernel, dim3(blocks), dim3(kStoreThreads), 0, st, a);
    HIPCHK(c, hipGetLastError());
  }
  if (dry) {
    if (a.n_ev) HIPCHK(c, hipMemcpyAsync(evicted, w.ev_ids.p, a.n_ev * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(tot, w.tot.p, sizeof tot, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return DSX_OK;
  }
  // ---- move, rebuild: from the first write-back on the store is in between -------
  auto rest = [&]() -> int {
    if (kept && moves) {
      // Windows are whole tiles of the gather's grid over the arena's addresses;
      // a window's gather writes bounce[0, ..) through a pointer shifted so that
      // arena offset D = ka T - skew lands on bounce.p (16-byte aligned, as D's
      // address is: the bounce has the arena's grid).
      const uint64_t skew = (uintptr_t)s->arena.p & 15;
      const uint64_t k0 = (first_off + skew) / T, k1 = (kept_bytes + skew + T - 1) / T;
      for (uint64_t ka = k0; ka < k1; ka += win / T) {
        const uint64_t kb = std::min<uint64_t>(ka + win / T, k1);
        const uint64_t lo = std::max<uint64_t>(first_off, ka * T > skew ? ka * T - skew : 0);
        const uint64_t hi = std::min<uint64_t>(kb * T - skew, kept_bytes);
        uint8_t* out = (uint8_t*)((uintptr_t)w.bounce.p + skew - ka * T);
        const int r = assemble_launch(c, a.segs, kept, out, hi, lo, hi, false);
        if (r) return r;
        HIPCHK(c, hipMemcpyAsync(s->arena.p + lo, out + lo, hi - lo, hipMemcpyDeviceToDevice, st));
      }
    }
    if (kept) {
      HIPCHK(c, hipMemcpyAsync(s->ids.p, w.pids.p, kept * 32, hipMemcpyDeviceToDevice, st));
      HIPCHK(c, hipMemcpyAsync(s->ends.p, w.pends.p, kept * 8, hipMemcpyDeviceToDevice, st));
      if (s->tracked)
        HIPCHK(c, hipMemcpyAsync(s->stamps.p, w.pstamps.p, kept * 8, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(c, hipMemsetAsync(s->slots.p, 0xFF, s->cap * sizeof(uint32_t), st));
    if (kept) {
      hipLaunchKernelGGL(store_reclaim_kernel, dim3(blocks_of(kept)), dim3(kStoreThreads), 0, st,
                         (const uint8_t*)s->ids.p, (u64)kept, s->slots.p, (u64)(s->cap - 1),
                         (u64)s->salt);
      HIPCHK(c, hipGetLastError());
    }
    if (a.n_ev) HIPCHK(c, hipMemcpyAsync(evicted, w.ev_ids.p, a.n_ev * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(tot, w.tot.p, sizeof tot, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return DSX_OK;
  };
  const int rc = rest();
  if (rc) {
    (void)hipStreamSynchronize(st);
    s->broken = true;
    return rc;
  }
  s->chunks = kept;
  s->bytes = kept_bytes;
  return DSX_OK;
}

// An accepted put or copy into a tracked store: every entry the call's IDs name
// takes one new clock value.  The launch is behind the append on the stream,
// so the table holds the appended entries (s->chunks counts them already).
// wait: the call has nothing else left to wait for.
int touch_accepted(dsx_ctx* c, dsx_store* s, const uint8_t* d_ids, uint64_t n, bool wait) {
  hipLaunchKernelGGL(store_touch_kernel, dim3(blocks_of(n)), dim3(kStoreThreads), 0, c->stream, d_ids,
                     (u64)n, view_of(s), s->stamps.p, (u64)next_stamp(s), (u64*)nullptr);
  HIPCHK(c, hipGetLastError());
  s->clock = next_stamp(s);
  if (wait) HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSX_OK;
}

}  // namespace

void store_release(dsx_ctx* c) {
  StoreScratch& t = c->store;
  for (dsx_store* s : t.live) free_store(s);
  t.live.clear();
}

extern "C" int dsx_store_create(dsx_ctx_t* c, uint64_t arena_bytes, uint64_t max_chunks,
                                dsx_store_t** out) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !out || max_chunks > kCallMaxN) return DSX_E_INVAL;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  dsx_store* s = new dsx_store;
  s->ctx = c;
  s->max_chunks = max_chunks;
  s->arena_bytes = arena_bytes;
  s->cap = idset_table_cap(max_chunks);
  s->salt = idset_next_salt();
  auto build = [&]() -> int {
    HIPCHK(c, s->ids.ensure(c->mem, max_chunks * 32));
    HIPCHK(c, s->ends.ensure(c->mem, max_chunks));
    HIPCHK(c, s->slots.ensure(c->mem, s->cap));
    HIPCHK(c, s->arena.ensure(c->mem, arena_bytes));
    HIPCHK(c, hipMemsetAsync(s->slots.p, 0xFF, s->cap * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSX_OK;
  };
  const int rc = build();
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    free_store(s);
    return rc == DSX_E_HIP ? DSX_E_NOMEM : rc;
  }
  c->store.live.push_back(s);
  *out = s;
  return DSX_OK;
}

extern "C" int dsx_store_destroy(dsx_ctx_t* c, dsx_store_t* s) {
  if (!c || !s) return DSX_E_INVAL;
  auto& live = c->store.live;
  auto it = std::find(live.begin(), live.end(), s);
  if (it == live.end()) return foreign_store(c, DSX_E_INVAL);
  live.erase(it);
  HIPCHK(c, hipSetDevice(c->device));
  (void)hipStreamSynchronize(c->stream);
  free_store(s);
  return DSX_OK;
}

extern "C" int dsx_store_count(const dsx_store_t* s, dsx_store_counts_t* out) {
  if (!s || !out) return DSX_E_INVAL;
  if (s->broken) return DSX_E_STATE;
  out->chunks = s->chunks;
  out->bytes = s->bytes;
  out->max_chunks = s->max_chunks;
  out->arena_bytes = s->arena_bytes;
  return DSX_OK;
}

extern "C" int dsx_store_arena(const dsx_store_t* s, const void** d_arena, uint64_t* used) {
  if (!s) return DSX_E_INVAL;
  if (s->broken) return DSX_E_STATE;
  if (d_arena) *d_arena = s->arena.p;
  if (used) *used = s->bytes;
  return DSX_OK;
}

extern "C" int dsx_store_put(dsx_ctx_t* c, dsx_store_t* s, const void* d_blob, uint64_t len,
                             const void* ids, const uint64_t* ends, uint64_t start, uint64_t n,
                             dsx_store_put_totals_t* totals, uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  const uint32_t f_ids = DSX_IDS_DEVICE, f_ends = DSX_ENDS_DEVICE;
  if (!c || !s) return DSX_E_INVAL;
  if (totals) *totals = dsx_store_put_totals_t{};
  if ((flags & ~(f_ids | f_ends)) != 0) return invalid(c, "unknown flag bit");
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (n > kCallMaxN) return invalid(c, "more chunks than a call takes (0xFFFFFFF0)");
  if (n && (!ids || !ends)) return invalid(c, "the IDs or the chunk ends are missing");
  if (len && !d_blob) return invalid(c, "the blob is missing");
  if (len > UINT64_MAX - (uintptr_t)d_blob) return invalid(c, "the blob wraps the address space");
  if (n == 0) return DSX_OK;
  if (overlaps(d_blob, len, s->arena.p, s->arena_bytes))
    return invalid(c, "the blob overlaps the store's arena");
  if (!(flags & f_ends)) {
    uint64_t prev = start;
    for (uint64_t i = 0; i < n; ++i) {
      if (ends[i] < prev || ends[i] > len)
        return invalid(c, "chunk ends must be non-decreasing, start <= ends[0], ends[n-1] <= len");
      prev = ends[i];
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  IdsetScratch& t = c->idset;
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;

  PutArgs a{};
  int rc = stage_ids(c, ids, n, (flags & f_ids) != 0, &a.ids);
  if (rc) return rc;
  rc = stage_ends(c, ends, n, (flags & f_ends) != 0, &a.ends);
  if (rc) return rc;
  const uint32_t blocks = blocks_of(n);
  const uint64_t cap = idset_table_cap(n);
  HIPCHK(c, grow(c, t.slots, cap));
  HIPCHK(c, grow(c, t.tot, kIdsetCounters));

  // ---- select, scan ------------------------------------------------------------
  a.salt = idset_next_salt();
  rc = idset_enqueue_build(c, a.ids, n, t.slots.p, cap, a.salt, t.tot.p);
  if (rc) return rc;
  a.start = start;
  a.n = n;
  a.len = len;
  a.blob = (const uint8_t*)d_blob;
  a.slots = t.slots.p;
  a.mask = cap - 1;
  a.dst = view_of(s);
  // ---- the one wait before any byte is copied ----------------------------------
  u64 tot[kStoreCounters] = {};
  rc = select_scan_wait(c, n, [&](uint32_t grid) -> int {
    a.flag = w.flag.p, a.blk = w.blk.p, a.tot = w.tot.p;
    hipLaunchKernelGGL(store_select_kernel, dim3(grid), dim3(kStoreThreads), 0, st, a);
    HIPCHK(c, hipGetLastError());
    return DSX_OK;
  }, tot);
  if (rc) return rc;
  if (tot[3]) return invalid(c, "chunk ends must be non-decreasing, start <= ends[0], ends[n-1] <= len");
  const uint64_t stored = tot[0], stored_bytes = tot[1], present = tot[2];
  if (totals) {
    totals->total = n;
    totals->stored = stored;
    totals->stored_bytes = stored_bytes;
    totals->present = present;
    totals->repeats = n - stored - present;
  }
  if (stored > s->max_chunks - s->chunks || stored_bytes > s->arena_bytes - s->bytes) {
    c->err = "the store is full: " + std::to_string(stored) + " chunks of " +
             std::to_string(stored_bytes) + " bytes do not fit";
    return DSX_E_CAPACITY;
  }
  if (!stored) return s->tracked ? touch_accepted(c, s, a.ids, n, true) : DSX_OK;
  // ---- append, copy ------------------------------------------------------------
  HIPCHK(c, grow(c, w.segs, 3 * stored));
  a.segs = reinterpret_cast<AsmSeg*>(w.segs.p);
  a.n_new = stored;
  hipLaunchKernelGGL(store_append_kernel<false>, dim3(blocks), dim3(kStoreThreads), 0, st, a);
  HIPCHK(c, hipGetLastError());
  rc = assemble_launch(c, a.segs, stored, s->arena.p, s->bytes + stored_bytes, s->bytes,
                       s->bytes + stored_bytes, false);
  if (rc) return rc;
  s->chunks += stored;  // (the launches are enqueued: the store has the chunks from here on)
  s->bytes += stored_bytes;
  if (s->tracked) {
    rc = touch_accepted(c, s, a.ids, n, false);
    if (rc) return rc;
  }
  HIPCHK(c, hipStreamSynchronize(st));
  return DSX_OK;
}

// ids[idx ? idx[i] : i], i < m, looked up into d_offs / d_sizes (device, may be
// null) with the missing count in w.tot[0]; enqueues only
static int enqueue_lookup(dsx_ctx* c, const dsx_store* s, const uint8_t* d_ids, const uint32_t* d_idx,
                          uint64_t m, uint64_t* d_offs, uint64_t* d_sizes) {
  StoreScratch& w = c->store;
  HIPCHK(c, grow(c, w.tot, kStoreCounters));
  HIPCHK(c, hipMemsetAsync(w.tot.p, 0, kStoreCounters * sizeof(u64), c->stream));
  hipLaunchKernelGGL(store_lookup_kernel, dim3(blocks_of(m)), dim3(kStoreThreads), 0, c->stream, d_ids,
                     d_idx, (u64)m, view_of(s), d_offs, d_sizes, w.tot.p);
  HIPCHK(c, hipGetLastError());
  return DSX_OK;
}

extern "C" int dsx_store_locate(dsx_ctx_t* c, const dsx_store_t* s, const void* ids, uint64_t n,
                                uint64_t* offs, uint64_t* sizes, uint64_t* n_missing,
                                uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  const uint32_t f_ids = DSX_IDS_DEVICE, f_out = DSX_OUT_DEVICE;
  if (!c || !s) return DSX_E_INVAL;
  if (n_missing) *n_missing = 0;
  if ((flags & ~(f_ids | f_out)) != 0) return invalid(c, "unknown flag bit");
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (n > kCallMaxN) return invalid(c, "more IDs than a call takes (0xFFFFFFF0)");
  if (n && !ids) return invalid(c, "the IDs are missing");
  if (n == 0) return DSX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;
  const uint8_t* d_ids = nullptr;
  int rc = stage_ids(c, ids, n, (flags & f_ids) != 0, &d_ids);
  if (rc) return rc;
  uint64_t* d_offs = offs;
  if (offs && (!(flags & f_out) || !aligned(offs, 8))) {
    HIPCHK(c, grow(c, w.offs, n));
    d_offs = (uint64_t*)w.offs.p;
  }
  uint64_t* d_sizes = sizes;
  if (sizes && (!(flags & f_out) || !aligned(sizes, 8))) {
    HIPCHK(c, grow(c, w.sizes, n));
    d_sizes = (uint64_t*)w.sizes.p;
  }
  rc = enqueue_lookup(c, s, d_ids, nullptr, n, d_offs, d_sizes);
  if (rc) return rc;
  if (offs && d_offs != offs) HIPCHK(c, hipMemcpyAsync(offs, d_offs, n * 8, hipMemcpyDefault, st));
  if (sizes && d_sizes != sizes)
    HIPCHK(c, hipMemcpyAsync(sizes, d_sizes, n * 8, hipMemcpyDefault, st));
  u64 miss = 0;
  HIPCHK(c, hipMemcpyAsync(&miss, w.tot.p, sizeof miss, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (n_missing) *n_missing = miss;
  return DSX_OK;
}

extern "C" int dsx_store_entries(dsx_ctx_t* c, const dsx_store_t* s, uint64_t first, uint64_t n,
                                 void* ids, uint64_t* ends, uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !s) return DSX_E_INVAL;
  if ((flags & ~DSX_OUT_DEVICE) != 0) return invalid(c, "unknown flag bit");
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (first > s->chunks || n > s->chunks - first)
    return invalid(c, "first + n is beyond the store's entries");
  if (n == 0) return DSX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  hipStream_t st = c->stream;
  if (ids) HIPCHK(c, hipMemcpyAsync(ids, s->ids.p + 32 * first, n * 32, hipMemcpyDefault, st));
  if (ends) HIPCHK(c, hipMemcpyAsync(ends, s->ends.p + first, n * 8, hipMemcpyDefault, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return DSX_OK;
}

extern "C" int dsx_store_resolve(dsx_ctx_t* c, const dsx_store_t* s, const void* ids, uint64_t n,
                                 dsx_plan_seg_t* segs, uint64_t nsegs, uint64_t* n_missing,
                                 uint64_t* n_wrong_size, uint32_t* first_bad, uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !s) return DSX_E_INVAL;
  if (n_missing) *n_missing = 0;
  if (n_wrong_size) *n_wrong_size = 0;
  if (first_bad) *first_bad = 0xFFFFFFFFu;
  if ((flags & ~DSX_IDS_DEVICE) != 0) return invalid(c, "unknown flag bit");
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (n > kCallMaxN) return invalid(c, "more IDs than a call takes (0xFFFFFFF0)");
  if ((n && !ids) || (nsegs && !segs)) return invalid(c, "the IDs or the segments are missing");
  try {
    std::vector<uint32_t> idx;    // the store segments' target positions ...
    std::vector<uint64_t> where;  // ... and their numbers in segs[]
    for (uint64_t i = 0; i < nsegs; ++i) {
      const dsx_plan_seg_t& g = segs[i];
      if ((uint64_t)g.first + g.count > n) {
        c->err = "segment " + std::to_string(i) + ": first + count is beyond the target's chunks";
        return DSX_E_INVAL;
      }
      if (g.source != DSX_SRC_STORE) continue;
      if (g.first >= n) {
        c->err = "segment " + std::to_string(i) + ": first names no target chunk";
        return DSX_E_INVAL;
      }
      idx.push_back(g.first);
      where.push_back(i);
    }
    const uint64_t m = idx.size();
    if (m == 0) return DSX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->err.clear();
    StoreScratch& w = c->store;
    hipStream_t st = c->stream;
    const uint8_t* d_ids = nullptr;
    int rc = stage_ids(c, ids, n, (flags & DSX_IDS_DEVICE) != 0, &d_ids);
    if (rc) return rc;
    HIPCHK(c, grow(c, w.idx, m));
    HIPCHK(c, grow(c, w.offs, m));
    HIPCHK(c, grow(c, w.sizes, m));
    HIPCHK(c, hipMemcpyAsync(w.idx.p, idx.data(), m * 4, hipMemcpyHostToDevice, st));
    rc = enqueue_lookup(c, s, d_ids, w.idx.p, m, (uint64_t*)w.offs.p, (uint64_t*)w.sizes.p);
    if (rc) return rc;
    std::vector<uint64_t> offs(m), sizes(m);
    HIPCHK(c, hipMemcpyAsync(offs.data(), w.offs.p, m * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(sizes.data(), w.sizes.p, m * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    uint64_t miss = 0, wrong = 0;
    uint32_t bad = 0xFFFFFFFFu;
    for (uint64_t k = 0; k < m; ++k) {
      const bool gone = offs[k] == UINT64_MAX;
      const bool other = !gone && sizes[k] != segs[where[k]].bytes;
      miss += gone;
      wrong += other;
      if (gone || other) bad = std::min(bad, idx[k]);
    }
    if (n_missing) *n_missing = miss;
    if (n_wrong_size) *n_wrong_size = wrong;
    if (first_bad) *first_bad = bad;
    if (miss || wrong) return DSX_OK;
    for (uint64_t k = 0; k < m; ++k) segs[where[k]].src_off = offs[k];
    return DSX_OK;
  } catch (const std::bad_alloc&) {
    return DSX_E_NOMEM;
  }
}

extern "C" int dsx_store_verify(dsx_ctx_t* c, const dsx_store_t* s, int algo, uint32_t* bad,
                                uint64_t cap, uint64_t* n_bad) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !s) return DSX_E_INVAL;
  if (n_bad) *n_bad = 0;
  if (algo != DSX_DIGEST_SHA512_256 && algo != DSX_DIGEST_SHA256)
    return invalid(c, "algo names no digest");
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (cap && !bad) return invalid(c, "the list of bad entries is missing");
  const uint64_t n = s->chunks;
  if (n == 0) return DSX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;
  HIPCHK(c, grow(c, w.vids, n * 32));
  HIPCHK(c, grow(c, w.flag, n));
  HIPCHK(c, grow(c, w.tot, kStoreCounters));
  DigestArgs da{};
  da.blob = s->arena.p;
  da.len = s->bytes;
  da.ends = s->ends.p;
  da.first_start = 0;
  da.n = n;
  da.ids = w.vids.p;
  int rc = launch_digest(c, da, n, algo);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(w.tot.p, 0, kStoreCounters * sizeof(u64), st));
  hipLaunchKernelGGL(store_compare_kernel, dim3(blocks_of(n)), dim3(kStoreThreads), 0, st,
                     (const uint8_t*)w.vids.p, (const uint8_t*)s->ids.p, (u64)n, w.flag.p, w.tot.p);
  HIPCHK(c, hipGetLastError());
  u64 count = 0;
  HIPCHK(c, hipMemcpyAsync(&count, w.tot.p, sizeof count, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (n_bad) *n_bad = count;
  if (!count || !cap) return DSX_OK;
  try {
    std::vector<uint8_t> flag(n);  // (something is wrong: one byte per entry crosses)
    HIPCHK(c, hipMemcpy(flag.data(), w.flag.p, n, hipMemcpyDeviceToHost));
    uint64_t k = 0;
    for (uint64_t e = 0; e < n && k < cap; ++e)
      if (flag[e]) bad[k++] = (uint32_t)e;
    return DSX_OK;
  } catch (const std::bad_alloc&) {
    return DSX_E_NOMEM;
  }
}

extern "C" int dsx_store_prune(dsx_ctx_t* c, dsx_store_t* s, const void* ids, uint64_t n,
                               uint64_t window, dsx_store_prune_totals_t* totals, uint32_t flags) {
  const uint32_t f_ids = DSX_IDS_DEVICE, f_rm = DSX_PRUNE_REMOVE;
  if (!c || !s) return DSX_E_INVAL;
  DSX_FLUSH_BEHIND(c);
  if (totals) *totals = dsx_store_prune_totals_t{};
  if ((flags & ~(f_ids | f_rm)) != 0) return invalid(c, "unknown flag bit");
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (n > kCallMaxN) return invalid(c, "more IDs than a call takes (0xFFFFFFF0)");
  if (n && !ids) return invalid(c, "the IDs are missing");
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  IdsetScratch& t = c->idset;
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;
  const uint64_t entries = s->chunks;

  // ---- mark, scan --------------------------------------------------------------
  PruneArgs a{};
  int rc = n ? stage_ids(c, ids, n, (flags & f_ids) != 0, &a.ids) : DSX_OK;
  if (rc) return rc;
  const uint64_t cap = idset_table_cap(n);
  HIPCHK(c, grow(c, t.slots, cap));
  HIPCHK(c, grow(c, t.tot, kIdsetCounters));
  a.salt = idset_next_salt();
  rc = idset_enqueue_build(c, a.ids, n, t.slots.p, cap, a.salt, t.tot.p);
  if (rc) return rc;
  a.slots = t.slots.p;
  a.n = n;
  a.mask = cap - 1;
  a.invert = (flags & f_rm) ? 1 : 0;
  a.st = view_of(s);
  // ---- the one wait before anything moves ---------------------------------------
  u64 tot[kStoreCounters] = {}, distinct = 0;
  rc = select_scan_wait(c, entries, [&](uint32_t grid) -> int {
    a.flag = w.flag.p, a.blk = w.blk.p, a.tot = w.tot.p;
    hipLaunchKernelGGL(store_mark_kernel, dim3(grid), dim3(kStoreThreads), 0, st, a);
    HIPCHK(c, hipGetLastError());
    return DSX_OK;
  }, tot, &distinct);
  if (rc) return rc;
  const uint64_t kept = tot[0], kept_bytes = tot[1];
  if (kept > entries || kept_bytes > s->bytes) return invalid(c, "the store's entries are inconsistent");
  const uint64_t removed = entries - kept;
  const uint64_t named = (flags & f_rm) ? removed : kept;  // the distinct IDs of ids[] the store held
  if (totals) {
    totals->entries = entries;
    totals->kept = kept;
    totals->kept_bytes = kept_bytes;
    totals->removed = removed;
    totals->removed_bytes = s->bytes - kept_bytes;
    totals->unmatched = distinct - named;
  }
  if (!removed) return DSX_OK;

  rc = compact_tail(c, s, a, kept, kept_bytes, tot, window, false, nullptr);
  if (rc) return rc;
  if (totals) {
    totals->moved = tot[4];
    totals->moved_bytes = tot[5];
  }
  return DSX_OK;
}

extern "C" int dsx_store_copy(dsx_ctx_t* c, dsx_store_t* dst, const dsx_store_t* src, const void* ids,
                              uint64_t n, dsx_store_copy_totals_t* totals, uint32_t flags) {
  const uint32_t f_ids = DSX_IDS_DEVICE, f_all = DSX_COPY_ALL;
  if (!c) return DSX_E_INVAL;
  if (!dst || !src || !totals) return invalid(c, "a store or the totals are missing");
  DSX_FLUSH_BEHIND(c);
  *totals = dsx_store_copy_totals_t{};
  totals->first_missing = UINT64_MAX;
  if ((flags & ~(f_ids | f_all)) != 0) return invalid(c, "unknown flag bit");
  if (dst == src) return invalid(c, "the source and the destination are the same store");
  if (!owns(c, dst) || !owns(c, src)) return foreign_store(c, DSX_E_INVAL);
  if (dst->broken || src->broken) return broken_store(c);
  const bool all = (flags & f_all) != 0;
  if (all && (ids || n)) return invalid(c, "copying all entries takes no IDs: ids == NULL and n == 0");
  if (n > kCallMaxN) return invalid(c, "more IDs than a call takes (0xFFFFFFF0)");
  if (n && !ids) return invalid(c, "the IDs are missing");
  if (all) n = src->chunks;
  totals->total = n;
  if (n == 0) return DSX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  IdsetScratch& t = c->idset;
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;

  PutArgs a{};
  a.ids = src->ids.p;
  int rc = all ? DSX_OK : stage_ids(c, ids, n, (flags & f_ids) != 0, &a.ids);
  if (rc) return rc;
  const uint32_t blocks = blocks_of(n);
  const uint64_t cap = idset_table_cap(n);
  HIPCHK(c, grow(c, w.srce, n));

  // ---- select, scan ------------------------------------------------------------
  a.n = n;
  a.all = all ? 1 : 0;
  if (!all) {
    HIPCHK(c, grow(c, t.slots, cap));
    HIPCHK(c, grow(c, t.tot, kIdsetCounters));
    a.salt = idset_next_salt();
    rc = idset_enqueue_build(c, a.ids, n, t.slots.p, cap, a.salt, t.tot.p);
    if (rc) return rc;
    a.slots = t.slots.p;
    a.mask = cap - 1;
  }
  a.src = view_of(src);
  a.dst = view_of(dst);
  a.srce = w.srce.p;
  // ---- the one wait before dst is written anywhere -------------------------------
  u64 tot[kStoreCounters] = {};
  rc = select_scan_wait(c, n, [&](uint32_t grid) -> int {
    a.flag = w.flag.p, a.blk = w.blk.p, a.tot = w.tot.p;
    HIPCHK(c, hipMemsetAsync(w.tot.p + 4, 0xFF, sizeof(u64), st));  // first_missing: none
    hipLaunchKernelGGL(store_copy_select_kernel, dim3(grid), dim3(kStoreThreads), 0, st, a);
    HIPCHK(c, hipGetLastError());
    return DSX_OK;
  }, tot);
  if (rc) return rc;
  const uint64_t copied = tot[0], copied_bytes = tot[1];
  totals->copied = copied;
  totals->copied_bytes = copied_bytes;
  totals->present = tot[2];
  totals->missing = tot[3];
  totals->first_missing = tot[4];
  totals->repeats = n - copied - tot[2] - tot[3];
  if (tot[3]) return DSX_OK;  // (the counts are the answer: nothing is copied)
  if (copied > dst->max_chunks - dst->chunks || copied_bytes > dst->arena_bytes - dst->bytes) {
    c->err = "the store is full: " + std::to_string(copied) + " chunks of " +
             std::to_string(copied_bytes) + " bytes do not fit";
    return DSX_E_CAPACITY;
  }
  if (!copied) return dst->tracked ? touch_accepted(c, dst, a.ids, n, true) : DSX_OK;
  // ---- append, copy ------------------------------------------------------------
  HIPCHK(c, grow(c, w.segs, 3 * copied));
  a.segs = reinterpret_cast<AsmSeg*>(w.segs.p);
  a.n_new = copied;
  hipLaunchKernelGGL(store_append_kernel<true>, dim3(blocks), dim3(kStoreThreads), 0, st, a);
  HIPCHK(c, hipGetLastError());
  rc = assemble_launch(c, a.segs, copied, dst->arena.p, dst->bytes + copied_bytes, dst->bytes,
                       dst->bytes + copied_bytes, false);
  if (rc) return rc;
  const bool carry = all && dst->chunks == 0 && dst->tracked && src->tracked;
  dst->chunks += copied;  // (the launches are enqueued: dst has the chunks from here on)
  dst->bytes += copied_bytes;
  if (carry) {
    // every entry of src into an empty store: entry e of dst is entry e of src, and keeps its stamp
    HIPCHK(c, hipMemcpyAsync(dst->stamps.p, src->stamps.p, copied * 8, hipMemcpyDeviceToDevice, st));
    dst->clock = src->clock;
  } else {
    if (dst->tracked) {
      rc = touch_accepted(c, dst, a.ids, n, false);
      if (rc) return rc;
    }
    if (src->tracked) {  // (the stamps are not what `const` promises of src: its entries and its arena)
      dsx_store* from = const_cast<dsx_store*>(src);
      hipLaunchKernelGGL(store_touch_source_kernel, dim3(blocks), dim3(kStoreThreads), 0, st,
                         (const uint8_t*)w.flag.p, (const uint32_t*)w.srce.p, (u64)n, from->stamps.p,
                         (u64)from->chunks, (u64)next_stamp(from));
      HIPCHK(c, hipGetLastError());
      from->clock = next_stamp(from);
    }
  }
  HIPCHK(c, hipStreamSynchronize(st));
  return DSX_OK;
}

// ---- use tracking and eviction (include/dsx.h has the contracts) ----------------------
namespace {

int untracked_store(dsx_ctx* c) {
  c->err = "the store does not track use: dsx_store_track comes first";
  return DSX_E_STATE;
}

}  // namespace

extern "C" int dsx_store_track(dsx_ctx_t* c, dsx_store_t* s) {
  if (!c || !s) return DSX_E_INVAL;
  DSX_FLUSH_BEHIND(c);
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (s->tracked) return DSX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  if (s->stamps.ensure(c->mem, s->max_chunks) != 0) return DSX_E_NOMEM;
  HIPCHK(c, hipMemsetAsync(s->stamps.p, 0, s->stamps.n * sizeof(uint64_t), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  s->tracked = true;
  s->clock = 0;
  return DSX_OK;
}

extern "C" int dsx_store_touch(dsx_ctx_t* c, dsx_store_t* s, const void* ids, uint64_t n,
                               uint64_t stamp, uint64_t* n_missing, uint32_t flags) {
  if (!c || !s) return DSX_E_INVAL;
  DSX_FLUSH_BEHIND(c);
  if (n_missing) *n_missing = 0;
  if ((flags & ~DSX_IDS_DEVICE) != 0) return invalid(c, "unknown flag bit");
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (!s->tracked) return untracked_store(c);
  if (n > kCallMaxN) return invalid(c, "more IDs than a call takes (0xFFFFFFF0)");
  if (n && !ids) return invalid(c, "the IDs are missing");
  if (n == 0) return DSX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;
  const uint8_t* d_ids = nullptr;
  const int rc = stage_ids(c, ids, n, (flags & DSX_IDS_DEVICE) != 0, &d_ids);
  if (rc) return rc;
  HIPCHK(c, grow(c, w.tot, kStoreCounters));
  HIPCHK(c, hipMemsetAsync(w.tot.p, 0, kStoreCounters * sizeof(u64), st));
  const uint64_t t = stamp == DSX_STAMP_NOW ? next_stamp(s) : stamp;
  hipLaunchKernelGGL(store_touch_kernel, dim3(blocks_of(n)), dim3(kStoreThreads), 0, st, d_ids, (u64)n,
                     view_of(s), s->stamps.p, (u64)t, w.tot.p);
  HIPCHK(c, hipGetLastError());
  u64 miss = 0;
  HIPCHK(c, hipMemcpyAsync(&miss, w.tot.p, sizeof miss, hipMemcpyDeviceToHost, st));
  s->clock = std::max<uint64_t>(s->clock, t);  // (the launch is enqueued: the stamps are the store's from here on)
  HIPCHK(c, hipStreamSynchronize(st));
  if (n_missing) *n_missing = miss;
  return DSX_OK;
}

extern "C" int dsx_store_stamps(dsx_ctx_t* c, const dsx_store_t* s, uint64_t first, uint64_t n,
                                uint64_t* stamps, uint64_t* clock, uint32_t flags) {
  if (!c || !s) return DSX_E_INVAL;
  DSX_FLUSH_BEHIND(c);
  if ((flags & ~DSX_OUT_DEVICE) != 0) return invalid(c, "unknown flag bit");
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (!s->tracked) return untracked_store(c);
  if (first > s->chunks || n > s->chunks - first)
    return invalid(c, "first + n is beyond the store's entries");
  if (clock) *clock = s->clock;
  if (n == 0 || !stamps) return DSX_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  HIPCHK(c, hipMemcpyAsync(stamps, s->stamps.p + first, n * 8, hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSX_OK;
}

extern "C" int dsx_store_evict(dsx_ctx_t* c, dsx_store_t* s, uint64_t need_bytes, uint64_t need_chunks,
                               const void* pin_ids, uint64_t n_pin, uint8_t* evicted_ids, uint64_t cap,
                               uint64_t window, dsx_store_evict_totals_t* totals, uint32_t flags) {
  const uint32_t f_ids = DSX_IDS_DEVICE, f_dry = DSX_EVICT_DRY;
  if (!c || !s) return DSX_E_INVAL;
  DSX_FLUSH_BEHIND(c);
  if (totals) *totals = dsx_store_evict_totals_t{};
  if ((flags & ~(f_ids | f_dry)) != 0) return invalid(c, "unknown flag bit");
  if (!owns(c, s)) return foreign_store(c, DSX_E_INVAL);
  if (s->broken) return broken_store(c);
  if (!s->tracked) return untracked_store(c);
  if (n_pin > kCallMaxN) return invalid(c, "more IDs than a call takes (0xFFFFFFF0)");
  if (n_pin && !pin_ids) return invalid(c, "the pinned IDs are missing");
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  IdsetScratch& t = c->idset;
  StoreScratch& w = c->store;
  hipStream_t st = c->stream;
  const uint64_t entries = s->chunks;
  const uint64_t room_bytes = s->arena_bytes - s->bytes, room_chunks = s->max_chunks - s->chunks;
  // what the victims have to free: the needs less the room that is there
  const uint64_t nb = need_bytes > room_bytes ? need_bytes - room_bytes : 0;
  const uint64_t nc = need_chunks > room_chunks ? need_chunks - room_chunks : 0;
  const bool select = nb || nc;  // (else the empty prefix: the pin launch alone, for the totals)
  const int passes = dsx_evict::passes_of(s->clock);

  // ---- pins, descent, boundary class, keep mask, scan ----------------------------
  EvictArgs ea{};
  int rc = n_pin ? stage_ids(c, pin_ids, n_pin, (flags & f_ids) != 0, &ea.pin_ids) : DSX_OK;
  if (rc) return rc;
  const uint32_t blocks = blocks_of(entries);
  const uint64_t pcap = idset_table_cap(n_pin);
  HIPCHK(c, grow(c, t.slots, pcap));
  HIPCHK(c, grow(c, t.tot, kIdsetCounters));
  ea.pin_salt = idset_next_salt();
  rc = idset_enqueue_build(c, ea.pin_ids, n_pin, t.slots.p, pcap, ea.pin_salt, t.tot.p);
  if (rc) return rc;
  ea.pin_slots = t.slots.p;
  ea.n_pin = n_pin;
  ea.pin_mask = pcap - 1;
  ea.st = view_of(s);
  ea.stamps = s->stamps.p;
  ea.need_chunks = nc;
  ea.need_bytes = nb;
  HIPCHK(c, grow(c, w.ev_pinned, entries));
  HIPCHK(c, grow(c, w.ev_sel, kEvictSel));
  HIPCHK(c, grow(c, w.ev_hist, 8 * 2 * (uint64_t)dsx_evict::kBuckets, false));
  HIPCHK(c, grow(c, w.ev_blk, 2 * (uint64_t)blocks));
  ea.pinned = w.ev_pinned.p;
  ea.sel = w.ev_sel.p;
  ea.cblk = w.ev_blk.p;
  u64 tot[kStoreCounters] = {}, sel[kEvictSel] = {};
  // ---- the one wait before anything moves ---------------------------------------
  rc = select_scan_wait(c, entries, [&](uint32_t grid) -> int {
    ea.flag = w.flag.p, ea.blk = w.blk.p, ea.tot = w.tot.p;
    const dim3 g(grid), b(kStoreThreads);
    HIPCHK(c, hipMemsetAsync(ea.sel, 0, kEvictSel * sizeof(u64), st));
    hipLaunchKernelGGL(evict_pin_kernel, g, b, 0, st, ea);
    HIPCHK(c, hipGetLastError());
    if (select) {
      HIPCHK(c, hipMemsetAsync(w.ev_hist.p, 0, (size_t)passes * 2 * dsx_evict::kBuckets * sizeof(u64), st));
      for (int p = 0; p < passes; ++p) {
        ea.level = passes - 1 - p;
        ea.first = p == 0;
        ea.hist = w.ev_hist.p + (size_t)p * 2 * dsx_evict::kBuckets;
        hipLaunchKernelGGL(evict_hist_kernel, g, b, 0, st, ea);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(evict_choose_kernel, dim3(1), b, 0, st, ea);
        HIPCHK(c, hipGetLastError());
      }
      hipLaunchKernelGGL(evict_class_kernel, g, b, 0, st, ea);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(block_array_scan_kernel<2>, dim3(1), dim3(kArrayScanThreads), 0, st, ea.cblk,
                         (u64)grid, (u64*)nullptr);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(evict_keep_kernel, g, b, 0, st, ea);
      HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(sel, ea.sel, sizeof sel, hipMemcpyDeviceToHost, st));
    return DSX_OK;
  }, tot);
  if (rc) return rc;
  if (totals) {
    totals->entries = entries;
    totals->kept = entries;
    totals->kept_bytes = s->bytes;
    totals->pinned = sel[kSelPinned];
    totals->evictable = sel[kSelEvictable];
    totals->evictable_bytes = sel[kSelEvictableBytes];
  }
  if (!select) return DSX_OK;
  if (sel[kSelEvictable] < nc || sel[kSelEvictableBytes] < nb) {
    c->err = "the store cannot make the room: " + std::to_string(sel[kSelEvictable]) + " unpinned chunks of " +
             std::to_string(sel[kSelEvictableBytes]) + " bytes, " + std::to_string(nc) + " chunks and " +
             std::to_string(nb) + " bytes are missing";
    return DSX_E_CAPACITY;
  }
  const uint64_t kept = tot[0], kept_bytes = tot[1];
  if (sel[kSelFailed] || kept >= entries || kept_bytes > s->bytes) {
    c->err = "the eviction's selection is inconsistent with the store's entries";
    return DSX_E_INTERNAL;
  }
  const uint64_t evicted = entries - kept;
  if (totals) {
    totals->kept = kept;
    totals->kept_bytes = kept_bytes;
    totals->evicted = evicted;
    totals->evicted_bytes = s->bytes - kept_bytes;
    totals->cutoff = sel[kSelPrefix];
  }
  PruneArgs a{};
  a.st = ea.st;
  a.flag = w.flag.p, a.blk = w.blk.p, a.tot = w.tot.p;
  a.n_ev = evicted_ids ? std::min<uint64_t>(cap, evicted) : 0;
  rc = compact_tail(c, s, a, kept, kept_bytes, tot, window, (flags & f_dry) != 0, evicted_ids);
  if (rc) return rc;
  if (totals) {
    totals->moved = tot[4];
    totals->moved_bytes = tot[5];
  }
  return DSX_OK;
}
