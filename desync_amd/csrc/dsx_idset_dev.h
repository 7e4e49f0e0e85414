// dsx_idset_dev.h -- the device side of the keyed open-addressing ID table,
// shared by the translation units whose kernels probe one (dsx_idset.hip: the
// sets; dsx_store.hip: the chunk store), and the host helpers that size, key
// and build a table.  The table's properties are stated in dsx_idset.hip.  The
// wave reductions the kernels count with are dsx_blockscan.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsx_blockscan.h"
#include "dsx_engine.h"

namespace dsx {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr int kIdsetThreads = 256;

struct Id32 {
  uint4 lo, hi;
};

__device__ __forceinline__ Id32 load_id(const uint8_t* ids, u64 i) {
  const uint4* p = reinterpret_cast<const uint4*>(ids + 32 * i);  // (ids is 16-byte aligned)
  Id32 r;
  r.lo = p[0];
  r.hi = p[1];
  return r;
}

__device__ __forceinline__ bool same_id(const Id32& a, const Id32& b) {
  const uint32_t d = (a.lo.x ^ b.lo.x) | (a.lo.y ^ b.lo.y) | (a.lo.z ^ b.lo.z) | (a.lo.w ^ b.lo.w) |
                     (a.hi.x ^ b.hi.x) | (a.hi.y ^ b.hi.y) | (a.hi.z ^ b.hi.z) | (a.hi.w ^ b.hi.w);
  return d == 0;
}

__device__ __forceinline__ u64 mix64(u64 x) {
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// every step is a bijection of the word it takes in: two IDs that differ in
// one word never share a hash before the mask
__device__ __forceinline__ u64 hash_id(const Id32& a, u64 salt) {
  u64 h = mix64(salt ^ ((u64)a.lo.y << 32 | a.lo.x));
  h = mix64(h ^ ((u64)a.lo.w << 32 | a.lo.z));
  h = mix64(h ^ ((u64)a.hi.y << 32 | a.hi.x));
  return mix64(h ^ ((u64)a.hi.w << 32 | a.hi.z));
}

__device__ __forceinline__ uint32_t idset_find(const uint8_t* ids, u64 n, const uint32_t* slots,
                                               u64 mask, u64 salt, const Id32& key) {
  u64 s = hash_id(key, salt) & mask;
  for (u64 step = 0; step <= mask; ++step, s = (s + 1) & mask) {
    const uint32_t j = slots[s];
    if (j == kEmpty) return kEmpty;
    if (j < n && same_id(load_id(ids, j), key)) return j;
  }
  return kEmpty;
}

// the entry of `key` in a store (dsx_store.h), or kEmpty
__device__ __forceinline__ uint32_t store_find(const StoreView& v, const Id32& key) {
  return idset_find(v.ids, v.n, v.slots, v.mask, v.salt, key);
}

// Claims for `entry` the first empty slot on id's probe sequence.  For IDs
// that differ from each other and from every ID the table holds: the IDs a put
// or a copy appends in one call (that is what its select selected), and a
// store's own entries claiming their slots in a cleared table.  No ID is
// compared: a comparison would read an entry another lane of the same launch
// is still writing.  No lane waits for another; the probe loop is bounded by
// the capacity.
__device__ __forceinline__ void idset_claim_empty(uint32_t* slots, u64 mask, u64 salt, const Id32& id,
                                                  uint32_t entry) {
  u64 s = hash_id(id, salt) & mask;
  for (u64 step = 0; step <= mask; ++step, s = (s + 1) & mask) {
    uint32_t cur = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur != kEmpty) continue;
    cur = atomicCAS(&slots[s], kEmpty, entry);
    if (cur == kEmpty) break;
  }
}

// One lane per ID.  *claimed counts the slots taken: the distinct IDs.
__global__ void idset_insert_kernel(const uint8_t* ids, u64 n, uint32_t* slots, u64 mask, u64 salt,
                                    u64* claimed);

}  // namespace dsx

// host side (dsx_idset.hip)
uint64_t idset_table_cap(uint64_t n);  // slots of a table over n IDs: a power of two >= 2 n
uint64_t idset_next_salt();            // a fresh hash key per table
// clears the table and the counters, then inserts ids[0..n) (device, 16-byte
// aligned); *tot[0] ends as the number of distinct IDs
int idset_enqueue_build(dsx_ctx* c, const uint8_t* d_ids, uint64_t n, uint32_t* slots, uint64_t cap,
                        uint64_t salt, dsx::u64* tot);
