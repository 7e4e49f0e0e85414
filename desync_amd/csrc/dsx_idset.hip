// dsx_idset.hip -- chunk-ID sets on the device: the dedup map of `desync info`
// (cmd/desync/info.go:135-150), the seed's first-position map
// (fileseed.go:24-36) and info.go's counters, over 32-byte IDs in HBM.
//
// The table is open addressing with linear probing over uint32 slots: a slot
// is kEmpty or a position in the ID array the table was built from.  The key
// of a full slot is ids[slot]; a slot never changes key, only (by atomicMin)
// to a lower position of the same key.  Equal IDs walk the same probe
// sequence, so every ID ends with exactly one slot, holding its lowest
// position, whatever the order the lanes arrive in: the result is exact and
// the same on every run.
//
// No lane waits for another (no spin, no flag): a lane either claims an empty
// slot, finds its own key, or steps on.  The probe loop is bounded by the
// capacity, and with a load factor <= 0.5 an empty slot always exists.
//
// The hash mixes all four 64-bit words of the ID with a per-table key: IDs
// come from index files and can be crafted, and a prefix hash (or a public
// unkeyed one) would let a crafted index line every ID up behind one slot.
//
// The device side of the table (the ID loads, the hash, the lookup) is in
// dsx_idset_dev.h: the chunk store (dsx_store.hip) keeps the same table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <random>

#include "dsx_callargs.h"
#include "dsx_engine.h"
#include "dsx_idset_dev.h"

namespace dsx {

// One lane per ID.  *claimed counts the slots taken: the distinct IDs.
__global__ __launch_bounds__(kIdsetThreads) void idset_insert_kernel(const uint8_t* ids, u64 n,
                                                                     uint32_t* slots, u64 mask,
                                                                     u64 salt, u64* claimed) {
  const u64 i = (u64)blockIdx.x * kIdsetThreads + threadIdx.x;
  bool took = false;
  if (i < n) {
    const Id32 me = load_id(ids, i);
    // a run of equal IDs (a zero run: every chunk the null chunk) is stood
    // for by its first lane, instead of one atomic per chunk on one word
    const bool run = i > 0 && same_id(me, load_id(ids, i - 1));
    if (!run) {
      u64 s = hash_id(me, salt) & mask;
      for (u64 step = 0; step <= mask; ++step, s = (s + 1) & mask) {
        uint32_t cur = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty) {
          cur = atomicCAS(&slots[s], kEmpty, (uint32_t)i);
          if (cur == kEmpty) {
            took = true;
            break;
          }
        }
        // occupied by position cur (< n: only positions are ever stored)
        if (cur < n && same_id(load_id(ids, cur), me)) {
          // the slot only ever falls: nothing to do unless this lane is lower
          if ((uint32_t)i < cur) atomicMin(&slots[s], (uint32_t)i);
          break;
        }
      }
    }
  }
  const u64 b = __ballot(took);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(claimed, (u64)__popcll(b));
}

struct ProbeArgs {
  const uint8_t* ids;      // the target's IDs
  const uint64_t* ends;    // chunk ends, or sizes
  u64 start, n;
  const uint32_t* slots;   // the target's table (built by the launch before)
  u64 mask, salt;
  const uint8_t* seed_ids;  // null: no seed
  const uint32_t* seed_slots;
  u64 seed_n, seed_mask, seed_salt;
  uint32_t* first_pos;     // may be null
  uint32_t* seed_pos;      // may be null
  u64* tot;                // [kIdsetCounters]
  int sizes;               // ends[] holds sizes
};

// A later launch on the same stream: the kernel boundary is the only ordering
// the tables need.  Totals: reduced in the wave, one atomic per wave per
// counter that is not zero.
__global__ __launch_bounds__(kIdsetThreads) void idset_probe_kernel(ProbeArgs a) {
  const u64 i = (u64)blockIdx.x * kIdsetThreads + threadIdx.x;
  bool first = false, in_seed = false;
  u64 size = 0;
  if (i < a.n) {
    const Id32 me = load_id(a.ids, i);
    const uint32_t fp = idset_find(a.ids, a.n, a.slots, a.mask, a.salt, me);
    uint32_t sp = kEmpty;
    if (a.seed_ids) sp = idset_find(a.seed_ids, a.seed_n, a.seed_slots, a.seed_mask, a.seed_salt, me);
    if (a.first_pos) a.first_pos[i] = fp;
    if (a.seed_pos) a.seed_pos[i] = sp;
    const u64 e = a.ends[i];
    size = a.sizes ? e : e - (i ? a.ends[i - 1] : a.start);
    first = fp == (uint32_t)i;
    in_seed = first && sp != kEmpty;
  }
  const u64 bf = __ballot(first), bs = __ballot(in_seed);
  const u64 sum_all = wave_sum(size);
  const u64 sum_new = wave_sum(first && !in_seed ? size : 0);
  if ((threadIdx.x & 63) == 0) {
    if (bf) atomicAdd(&a.tot[0], (u64)__popcll(bf));
    if (bs) atomicAdd(&a.tot[1], (u64)__popcll(bs));
    if (sum_all) atomicAdd(&a.tot[2], sum_all);
    if (sum_new) atomicAdd(&a.tot[3], sum_new);
  }
}

// dsx_seed_plan's classes: cls[i] = the lowest position in the seed of ids[i]'s
// ID (kEmpty: not held); with is_null non-null, also whether ids[i] is null_id.
__global__ __launch_bounds__(kIdsetThreads) void idset_class_kernel(
    const uint8_t* ids, u64 n, const uint8_t* seed_ids, const uint32_t* seed_slots, u64 seed_n,
    u64 seed_mask, u64 seed_salt, uint32_t* cls, Id32 null_id, uint8_t* is_null) {
  const u64 i = (u64)blockIdx.x * kIdsetThreads + threadIdx.x;
  if (i >= n) return;
  const Id32 me = load_id(ids, i);
  if (cls) cls[i] = idset_find(seed_ids, seed_n, seed_slots, seed_mask, seed_salt, me);
  if (is_null) is_null[i] = same_id(me, null_id) ? 1 : 0;
}

}  // namespace dsx

using namespace dsx;

uint64_t idset_table_cap(uint64_t n) {
  uint64_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}

// a fresh hash key per table (splitmix64 of a counter from a random origin)
uint64_t idset_next_salt() {
  static std::atomic<uint64_t> ctr{[] {
    std::random_device rd;
    return ((uint64_t)rd() << 32) ^ rd();
  }()};
  uint64_t z = ctr.fetch_add(0x9E3779B97F4A7C15ull) + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// clears the table and the counters, then inserts ids[0..n) (device, 16-byte
// aligned); *tot[0] ends as the number of distinct IDs
int idset_enqueue_build(dsx_ctx* c, const uint8_t* d_ids, uint64_t n, uint32_t* slots, uint64_t cap,
                        uint64_t salt, u64* tot) {
  HIPCHK(c, hipMemsetAsync(slots, 0xFF, cap * sizeof(uint32_t), c->stream));
  HIPCHK(c, hipMemsetAsync(tot, 0, kIdsetCounters * sizeof(u64), c->stream));
  if (!n) return DSX_OK;
  const uint32_t blocks = (uint32_t)((n + kIdsetThreads - 1) / kIdsetThreads);
  hipLaunchKernelGGL(idset_insert_kernel, dim3(blocks), dim3(kIdsetThreads), 0, c->stream, d_ids,
                     (u64)n, slots, (u64)(cap - 1), (u64)salt, tot);
  HIPCHK(c, hipGetLastError());
  return DSX_OK;
}

namespace {

void free_set(dsx_idset* s) {
  s->ids.release();
  s->slots.release();
  s->sclass.release();
  delete s;
}

}  // namespace

void idset_release(dsx_ctx* c) {
  IdsetScratch& t = c->idset;
  for (dsx_idset* s : t.live) free_set(s);
  t.live.clear();
}

extern "C" int dsx_idset_create(dsx_ctx_t* c, const void* ids, uint64_t n, uint32_t flags,
                                dsx_idset_t** out) {
  DSX_FLUSH_BEHIND(c);
  const uint32_t known = DSX_IDS_DEVICE;
  if (!c || !out || (n && !ids) || (flags & ~known) != 0 || n > kCallMaxN) return DSX_E_INVAL;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  IdsetScratch& t = c->idset;
  dsx_idset* s = new dsx_idset;
  s->ctx = c;
  s->n = n;
  s->cap = idset_table_cap(n);
  s->salt = idset_next_salt();
  int rc = DSX_OK;
  auto build = [&]() -> int {
    HIPCHK(c, s->ids.ensure(c->mem, n * 32));
    HIPCHK(c, s->slots.ensure(c->mem, s->cap));
    HIPCHK(c, t.tot.ensure(c->mem, kIdsetCounters));
    const hipMemcpyKind kind = (flags & known) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (n) HIPCHK(c, hipMemcpyAsync(s->ids.p, ids, n * 32, kind, c->stream));
    const int r = idset_enqueue_build(c, s->ids.p, n, s->slots.p, s->cap, s->salt, t.tot.p);
    if (r) return r;
    u64 uniq = 0;
    HIPCHK(c, hipMemcpyAsync(&uniq, t.tot.p, sizeof uniq, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s->n_unique = uniq;
    return DSX_OK;
  };
  rc = build();
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    free_set(s);
    return rc;
  }
  t.live.push_back(s);
  *out = s;
  return DSX_OK;
}

extern "C" int dsx_idset_destroy(dsx_ctx_t* c, dsx_idset_t* s) {
  if (!c || !s) return DSX_E_INVAL;
  auto& live = c->idset.live;
  auto it = std::find(live.begin(), live.end(), s);
  if (it == live.end()) return DSX_E_INVAL;  // (not a set of this context)
  live.erase(it);
  HIPCHK(c, hipSetDevice(c->device));
  (void)hipStreamSynchronize(c->stream);
  free_set(s);
  return DSX_OK;
}

extern "C" int dsx_idset_count(const dsx_idset_t* s, uint64_t* n_ids, uint64_t* n_unique) {
  if (!s) return DSX_E_INVAL;
  if (n_ids) *n_ids = s->n;
  if (n_unique) *n_unique = s->n_unique;
  return DSX_OK;
}

extern "C" int dsx_dedup(dsx_ctx_t* c, const void* ids, const uint64_t* ends, uint64_t start,
                         uint64_t n, const dsx_idset_t* seed, uint32_t* first_pos,
                         uint32_t* seed_pos, dsx_dedup_totals_t* totals, uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  const uint32_t f_ids = DSX_IDS_DEVICE, f_ends = DSX_ENDS_DEVICE, f_out = DSX_OUT_DEVICE,
                 f_sizes = DSX_SIZES;
  if (!c || (flags & ~(f_ids | f_ends | f_out | f_sizes)) != 0) return DSX_E_INVAL;
  if (n > kCallMaxN || (n && (!ids || !ends))) return DSX_E_INVAL;
  if (seed && seed->ctx != c) {
    c->err = "the seed set belongs to another context";
    return DSX_E_INVAL;
  }
  if (totals) *totals = dsx_dedup_totals_t{};
  if (n == 0) return DSX_OK;
  const bool sizes = (flags & f_sizes) != 0;
  if (!(flags & f_ends) && !sizes) {
    uint64_t prev = start;
    for (uint64_t i = 0; i < n; ++i) {
      if (ends[i] < prev) {
        c->err = "chunk ends must be non-decreasing, with start <= ends[0]";
        return DSX_E_INVAL;
      }
      prev = ends[i];
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->err.clear();
  IdsetScratch& t = c->idset;
  hipStream_t st = c->stream;

  // arguments the kernels cannot read in place (host memory, or a device
  // pointer below the vector loads' alignment) are staged in the context
  const uint8_t* d_ids = nullptr;
  const uint64_t* d_ends = nullptr;
  int rc = stage_ids(c, ids, n, (flags & f_ids) != 0, &d_ids);
  if (!rc) rc = stage_ends(c, ends, n, (flags & f_ends) != 0, &d_ends);
  if (rc) return rc;
  uint32_t* d_first = first_pos;
  if (first_pos && (!(flags & f_out) || !aligned(first_pos, 4))) {
    HIPCHK(c, grow(c, t.first_pos, n));
    d_first = t.first_pos.p;
  }
  uint32_t* d_seed = seed_pos;
  if (seed_pos && (!(flags & f_out) || !aligned(seed_pos, 4))) {
    HIPCHK(c, grow(c, t.seed_pos, n));
    d_seed = t.seed_pos.p;
  }
  const uint64_t cap = idset_table_cap(n);
  HIPCHK(c, grow(c, t.slots, cap));
  HIPCHK(c, grow(c, t.tot, kIdsetCounters));
  const uint64_t salt = idset_next_salt();
  rc = idset_enqueue_build(c, d_ids, n, t.slots.p, cap, salt, t.tot.p);
  if (rc) return rc;
  // (the insert left the distinct count in tot[0]; the probe counts it again
  // from first_pos, so start it from zero)
  HIPCHK(c, hipMemsetAsync(t.tot.p, 0, sizeof(u64), st));

  ProbeArgs a{};
  a.ids = d_ids;
  a.ends = d_ends;
  a.start = start;
  a.n = n;
  a.slots = t.slots.p;
  a.mask = cap - 1;
  a.salt = salt;
  if (seed) {
    a.seed_ids = seed->ids.p;
    a.seed_slots = seed->slots.p;
    a.seed_n = seed->n;
    a.seed_mask = seed->cap - 1;
    a.seed_salt = seed->salt;
  }
  a.first_pos = d_first;
  a.seed_pos = d_seed;
  a.tot = t.tot.p;
  a.sizes = sizes ? 1 : 0;
  const uint32_t blocks = (uint32_t)((n + kIdsetThreads - 1) / kIdsetThreads);
  hipLaunchKernelGGL(idset_probe_kernel, dim3(blocks), dim3(kIdsetThreads), 0, st, a);
  HIPCHK(c, hipGetLastError());

  if (first_pos && d_first != first_pos)
    HIPCHK(c, hipMemcpyAsync(first_pos, d_first, n * 4, hipMemcpyDefault, st));
  if (seed_pos && d_seed != seed_pos)
    HIPCHK(c, hipMemcpyAsync(seed_pos, d_seed, n * 4, hipMemcpyDefault, st));
  u64 tot[kIdsetCounters] = {};
  HIPCHK(c, hipMemcpyAsync(tot, t.tot.p, sizeof tot, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (totals) {
    totals->total = n;
    totals->unique = tot[0];
    totals->in_seed = tot[1];
    totals->size = start + tot[2];
    totals->size_not_in_seed = tot[3];
  }
  return DSX_OK;
}

// ---- the plan from IDs (SeedSequencer.Plan, sequencer.go:41-74) ----------------
// The classes dsx_plan_walk needs are what the tables already answer: a seed's
// table probed with the target's IDs gives tclass, probed with the seed's own
// IDs sclass (kept in the set), and dsx_dedup first_pos.  They cross to the
// host as 4 bytes per chunk per seed; the walk itself is host code.
extern "C" int dsx_seed_plan(dsx_ctx_t* c, const void* ids, const uint64_t* ends, uint64_t start,
                             uint64_t n, dsx_idset_t* const* seeds,
                             const uint64_t* const* seed_ends, const uint64_t* seed_counts,
                             uint32_t nseeds, const uint8_t* null_id, uint32_t limit,
                             dsx_plan_seg_t* segs, uint64_t seg_cap, uint32_t* store_chunks,
                             uint64_t store_cap, dsx_plan_totals_t* totals, uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  const uint32_t f_ids = DSX_IDS_DEVICE, f_ends = DSX_ENDS_DEVICE;
  if (!c || !totals || (flags & ~(f_ids | f_ends)) != 0) return DSX_E_INVAL;
  if (n > kCallMaxN || (n && (!ids || !ends))) return DSX_E_INVAL;
  if (nseeds && (!seeds || !seed_ends || !seed_counts)) return DSX_E_INVAL;
  *totals = dsx_plan_totals_t{};
  IdsetScratch& t = c->idset;
  for (uint32_t k = 0; k < nseeds; ++k) {
    dsx_idset* s = seeds[k];
    if (!s || std::find(t.live.begin(), t.live.end(), s) == t.live.end()) {
      c->err = "seed " + std::to_string(k) + " is not a set of this context";
      return DSX_E_INVAL;
    }
    if (seed_counts[k] != s->n || (s->n && !seed_ends[k])) {
      c->err = "seed " + std::to_string(k) + ": the number of chunk ends differs from the set's IDs";
      return DSX_E_INVAL;
    }
  }
  if (n == 0) return DSX_OK;
  try {
    std::vector<uint32_t> first_pos(n);
    int rc = dsx_dedup(c, ids, ends, start, n, nullptr, first_pos.data(), nullptr, nullptr, flags);
    if (rc) return rc;
    hipStream_t st = c->stream;
    // (dsx_dedup staged the IDs it could not read in place; they are still there)
    const uint8_t* d_ids = (const uint8_t*)ids;
    if (!(flags & f_ids) || !aligned(ids, 16)) d_ids = t.ids.p;
    std::vector<uint64_t> h_ends;
    if (flags & f_ends) {
      h_ends.resize(n);
      HIPCHK(c, hipMemcpyAsync(h_ends.data(), ends, n * 8, hipMemcpyDeviceToHost, st));
      ends = h_ends.data();
    }
    Id32 nid{};
    if (null_id) memcpy(&nid, null_id, 32);
    auto classes = [&](const uint8_t* of, uint64_t cnt, const dsx_idset* s, uint32_t* cls,
                       uint8_t* isn) -> int {
      const uint32_t blocks = (uint32_t)((cnt + kIdsetThreads - 1) / kIdsetThreads);
      hipLaunchKernelGGL(idset_class_kernel, dim3(blocks), dim3(kIdsetThreads), 0, st, of, (u64)cnt,
                         s ? s->ids.p : nullptr, s ? s->slots.p : nullptr, (u64)(s ? s->n : 0),
                         (u64)(s ? s->cap - 1 : 0), (u64)(s ? s->salt : 0), cls, nid, isn);
      HIPCHK(c, hipGetLastError());
      return DSX_OK;
    };
    // each seed's own classes, once per set
    for (uint32_t k = 0; k < nseeds; ++k) {
      dsx_idset* s = seeds[k];
      if (!s->n || s->h_sclass.size() == s->n) continue;
      HIPCHK(c, s->sclass.ensure(c->mem, s->n));
      if ((rc = classes(s->ids.p, s->n, s, s->sclass.p, nullptr))) return rc;
      std::vector<uint32_t> h(s->n);
      HIPCHK(c, hipMemcpyAsync(h.data(), s->sclass.p, s->n * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
      s->h_sclass.swap(h);
    }
    std::vector<uint8_t> is_null;
    if (null_id) {
      is_null.resize(n);
      HIPCHK(c, grow(c, t.is_null, n));
    }
    HIPCHK(c, grow(c, t.seed_pos, n));
    std::vector<std::vector<uint32_t>> tcls(nseeds);
    for (uint32_t k = 0; k < nseeds || (k == 0 && null_id); ++k) {
      uint8_t* isn = (k == 0 && null_id) ? t.is_null.p : nullptr;
      const dsx_idset* s = k < nseeds ? seeds[k] : nullptr;
      if ((rc = classes(d_ids, n, s, s ? t.seed_pos.p : nullptr, isn))) return rc;
      if (s) {
        tcls[k].resize(n);
        HIPCHK(c, hipMemcpyAsync(tcls[k].data(), t.seed_pos.p, n * 4, hipMemcpyDeviceToHost, st));
      }
      if (isn) HIPCHK(c, hipMemcpyAsync(is_null.data(), isn, n, hipMemcpyDeviceToHost, st));
      // (the next seed's launch overwrites seed_pos: the copy is stream-ordered before it)
    }
    HIPCHK(c, hipStreamSynchronize(st));
    std::vector<dsx_plan_seed_t> ps(nseeds);
    for (uint32_t k = 0; k < nseeds; ++k) {
      ps[k].tclass = tcls[k].data();
      ps[k].sclass = seeds[k]->h_sclass.data();
      ps[k].ends = seed_ends[k];
      ps[k].m = seeds[k]->n;
    }
    rc = dsx_plan_walk(ends, start, n, first_pos.data(), null_id ? is_null.data() : nullptr,
                       ps.data(), nseeds, limit, segs, seg_cap, store_chunks, store_cap, totals);
    if (rc == DSX_E_INVAL) c->err = "the chunk lists are not well formed (ends that decrease)";
    return rc;
  } catch (const std::bad_alloc&) {
    return DSX_E_NOMEM;
  }
}
