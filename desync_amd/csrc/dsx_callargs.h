// dsx_callargs.h -- what the C-ABI calls over chunk IDs, chunk ends and stores
// (dsx_idset.hip, dsx_store.hip, dsx_read.hip, dsx_assemble.hip, dsx_aead.hip)
// share on the host: the call limit, the pointer checks, the refusals of a
// store, and the staging of IDs and ends a kernel cannot read in place.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>

#include "dsx_engine.h"

// items (IDs, chunks, ranges, (range, chunk) pairs) a call takes: positions
// and entry numbers are 32 bits, 0xFFFFFFFF is the empty slot
constexpr uint64_t kCallMaxN = 0xFFFFFFF0ull;

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// [a, a + an) and [b, b + bn) share a byte
inline bool overlaps(const void* a, uint64_t an, const void* b, uint64_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return an && bn && x < y + bn && y < x + an;
}

inline int invalid(dsx_ctx* c, const std::string& what) {
  c->err = what;
  return DSX_E_INVAL;
}

inline bool owns(const dsx_ctx* c, const dsx_store* s) {
  const auto& live = c->store.live;
  return std::find(live.begin(), live.end(), s) != live.end();
}

// a store !owns(): the dsx_store_* calls answer DSX_E_INVAL, dsx_read_ranges DSX_E_STATE
inline int foreign_store(dsx_ctx* c, int code) {
  c->err = "the store belongs to another context";
  return code;
}

inline int broken_store(dsx_ctx* c) {
  c->err = "the store is broken: a prune failed while it moved the arena; destroy it";
  return DSX_E_STATE;
}

// The n IDs (n > 0) where a kernel can read them: in place (device memory,
// aligned for the 16-byte loads), or staged in the context on its stream.
inline int stage_ids(dsx_ctx* c, const void* ids, uint64_t n, bool device, const uint8_t** out) {
  *out = (const uint8_t*)ids;
  if (device && aligned(ids, 16)) return DSX_OK;
  IdsetScratch& t = c->idset;
  HIPCHK(c, grow(c, t.ids, n * 32));
  HIPCHK(c, hipMemcpyAsync(t.ids.p, ids, n * 32, hipMemcpyDefault, c->stream));
  *out = t.ids.p;
  return DSX_OK;
}

// the n chunk ends (n > 0), likewise
inline int stage_ends(dsx_ctx* c, const uint64_t* ends, uint64_t n, bool device, const uint64_t** out) {
  *out = ends;
  if (device && aligned(ends, 8)) return DSX_OK;
  IdsetScratch& t = c->idset;
  HIPCHK(c, grow(c, t.ends, n));
  HIPCHK(c, hipMemcpyAsync(t.ends.p, ends, n * 8, hipMemcpyDefault, c->stream));
  *out = t.ends.p;
  return DSX_OK;
}
