// dsx_plan.cpp -- SeedSequencer.Plan (sequencer.go:41-74) over 32-bit classes:
// dsx_plan_walk of include/dsx.h.  Host code only; nothing of HIP is included,
// so a plain C++ compiler builds this file alone (the sanitizer replay of
// tests/plan_replay.cpp does).
//
// The reference matches chunk IDs through a map ID -> positions
// (fileseed.go:24-36) and walks every occurrence chunk by chunk
// (maxMatchFrom, fileseed.go:114-136).  Here IDs are classes (the lowest
// position of the ID in the seed), and runs of one class are stepped over a
// run at a time:
//   trun[i] / srun[p]  the number of positions from i / p on with the class
//                      of i / p (the rest of its run);
//   extending a match at (i, p) with a = trun[i], b = srun[p]: if a != b one
//   side leaves its run after min(a, b) chunks while the other stays in it,
//   so the match ends there; if a == b both runs end together and the match
//   continues behind them;
//   of the positions inside one seed run [s, s + B) facing a target run of a,
//   p = s matches min(a, B) chunks (and more only if B == a), p = s + B - a
//   (B > a) matches a chunks and whatever follows both runs, every other p
//   matches no more than p = s: only those two can win under the reference's
//   ascending order and strictly-greater rule;
//   next[s]  the start of the next seed run of the same class, built by one
//   backward pass: the occurrence list, a run at a time.
// Periodic inputs (ABAB...) have runs of one chunk and cost what they cost in
// the reference.
#include <stdint.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/dsx.h"
#include "dsx_inplace_plan.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kMaxN = 0xFFFFFFF0ull;

struct SeedIx {
  const uint32_t* tclass;
  const uint32_t* sclass;
  const uint64_t* ends;
  uint32_t m;
  std::vector<uint32_t> trun, srun, next;
};

// the rest of the run of equal words each position starts
void run_lengths(const uint32_t* cls, uint32_t n, std::vector<uint32_t>& run) {
  run.resize(n);
  for (uint32_t i = n; i-- > 0;)
    run[i] = (i + 1 < n && cls[i + 1] == cls[i]) ? run[i + 1] + 1 : 1;
}

// chunks matching from target i and seed p on (maxMatchFrom), at most cap
uint64_t match_from(const SeedIx& s, uint32_t n, uint32_t i, uint32_t p, uint64_t cap) {
  uint64_t len = 0;
  while (i < n && p < s.m && len < cap && s.tclass[i] == s.sclass[p]) {
    const uint32_t a = s.trun[i], b = s.srun[p];
    if (a != b) {
      len += std::min(a, b);
      break;
    }
    len += a;
    i += a;  // (a <= n - i and a <= m - p: runs end inside their arrays)
    p += a;
  }
  return std::min(len, cap);
}

// FileSeed.LongestMatchWith at target position cur: the chunk count, *pos the
// seed position it starts at
uint64_t longest_match(const SeedIx& s, uint32_t n, uint32_t cur, uint32_t limit, uint32_t* pos) {
  const uint32_t c = s.tclass[cur];
  if (c == kNone || s.m == 0) return 0;
  const uint64_t cap = limit ? limit : UINT64_MAX;
  const uint32_t a = s.trun[cur];
  uint64_t best = 0;
  // c is the lowest position of its class, so it starts that class's first run
  for (uint32_t r = c; r != kNone; r = s.next[r]) {
    const uint32_t B = s.srun[r];
    uint32_t cand[2] = {r, kNone};
    if (B > a) cand[1] = r + (B - a);
    for (uint32_t p : cand) {
      if (p == kNone) continue;
      const uint64_t k = match_from(s, n, cur, p, cap);
      if (k > best) {
        best = k;
        *pos = p;
      }
      if (limit && best == limit) return best;  // (fileseed.go:75-77)
    }
  }
  return best;
}

}  // namespace

extern "C" int dsx_plan_walk(const uint64_t* ends, uint64_t start, uint64_t n,
                             const uint32_t* first_pos, const uint8_t* is_null,
                             const dsx_plan_seed_t* seeds, uint32_t nseeds, uint32_t limit,
                             dsx_plan_seg_t* segs, uint64_t seg_cap, uint32_t* store_chunks,
                             uint64_t store_cap, dsx_plan_totals_t* totals) {
  if (!totals || n > kMaxN || (nseeds && !seeds)) return DSX_E_INVAL;
  *totals = dsx_plan_totals_t{};
  if (n && (!ends || !first_pos)) return DSX_E_INVAL;
  if ((seg_cap && !segs) || (store_cap && !store_chunks)) return DSX_E_INVAL;
  const uint32_t N = (uint32_t)n;
  try {
    // ---- input checks: nothing below indexes outside an array ---------------
    uint64_t prev = start;
    for (uint32_t i = 0; i < N; ++i) {
      if (ends[i] < prev || first_pos[i] > i) return DSX_E_INVAL;
      prev = ends[i];
    }
    std::vector<SeedIx> ix(nseeds);
    for (uint32_t k = 0; k < nseeds; ++k) {
      const dsx_plan_seed_t& in = seeds[k];
      if (in.m > kMaxN) return DSX_E_INVAL;
      if ((in.m && (!in.sclass || !in.ends)) || (N && !in.tclass)) return DSX_E_INVAL;
      SeedIx& s = ix[k];
      s.tclass = in.tclass, s.sclass = in.sclass, s.ends = in.ends, s.m = (uint32_t)in.m;
      prev = 0;
      for (uint32_t p = 0; p < s.m; ++p) {
        const uint32_t c = s.sclass[p];
        if (c > p || s.sclass[c] != c || s.ends[p] < prev) return DSX_E_INVAL;
        prev = s.ends[p];
      }
      for (uint32_t i = 0; i < N; ++i) {
        const uint32_t c = s.tclass[i];
        if (c != kNone && (c >= s.m || s.sclass[c] != c)) return DSX_E_INVAL;
      }
    }
    if (N == 0) return DSX_OK;

    // ---- run lengths and the per-class list of seed runs --------------------
    for (SeedIx& s : ix) {
      run_lengths(s.tclass, N, s.trun);
      run_lengths(s.sclass, s.m, s.srun);
      s.next.assign(s.m, kNone);
      std::vector<uint32_t> head(s.m, kNone);  // per class: the lowest run start seen so far
      for (uint32_t p = s.m; p-- > 0;) {
        if (p > 0 && s.sclass[p - 1] == s.sclass[p]) continue;  // not a run start
        const uint32_t c = s.sclass[p];
        s.next[p] = head[c];
        head[c] = p;
      }
    }
    std::vector<uint32_t> nullrun;
    if (is_null) {
      nullrun.resize(N);
      for (uint32_t i = N; i-- > 0;)
        nullrun[i] = is_null[i] ? ((i + 1 < N) ? nullrun[i + 1] : 0) + 1 : 0;
    }
    // packed-store offset per ID of the target (indexed by first_pos), set at
    // the ID's first store segment
    std::vector<uint64_t> store_off;

    // ---- SeedSequencer.Plan -------------------------------------------------
    auto chunk_start = [&](uint32_t i) { return i ? ends[i - 1] : start; };
    dsx_plan_totals_t t{};
    for (uint32_t cur = 0; cur < N;) {
      uint64_t max = 0, advance = 1;
      int32_t source = DSX_SRC_STORE;
      uint32_t seed_first = kNone;
      if (is_null && nullrun[cur]) {
        const uint64_t k = limit ? std::min<uint64_t>(nullrun[cur], limit) : nullrun[cur];
        const uint64_t size = ends[cur + k - 1] - chunk_start(cur);
        if (size > max) source = DSX_SRC_NULL, advance = k, max = size;
      }
      for (uint32_t si = 0; si < nseeds; ++si) {
        const SeedIx& s = ix[si];
        uint32_t p = 0;
        const uint64_t k = longest_match(s, N, cur, limit, &p);
        if (!k) continue;
        const uint64_t size = s.ends[p + k - 1] - (p ? s.ends[p - 1] : 0);
        if (size > max) source = (int32_t)si, seed_first = p, advance = k, max = size;
      }
      dsx_plan_seg_t g{};
      g.dst_off = chunk_start(cur);
      g.bytes = ends[cur + advance - 1] - g.dst_off;
      g.first = cur;
      g.count = (uint32_t)advance;
      g.source = source;
      g.seed_first = seed_first;
      if (source >= 0) {
        g.src_off = seed_first ? ix[source].ends[seed_first - 1] : 0;
        t.seed_chunks += advance, t.seed_bytes += g.bytes;
      } else if (source == DSX_SRC_NULL) {
        t.null_chunks += advance, t.null_bytes += g.bytes;
      } else {
        if (store_off.empty()) store_off.assign(N, UINT64_MAX);
        uint64_t& off = store_off[first_pos[cur]];
        if (off == UINT64_MAX) {
          off = t.store_len;
          if (t.store_unique < store_cap) store_chunks[t.store_unique] = cur;
          ++t.store_unique;
          t.store_len += g.bytes;
        }
        g.src_off = off;
        t.store_chunks += 1, t.store_bytes += g.bytes;
      }
      if (t.segments < seg_cap) segs[t.segments] = g;
      ++t.segments;
      cur += (uint32_t)advance;
    }
    *totals = t;
    return (t.segments > seg_cap || t.store_unique > store_cap) ? DSX_E_CAPACITY : DSX_OK;
  } catch (const std::bad_alloc&) {
    return DSX_E_NOMEM;
  }
}

// The schedule of an in-place assembly (dsx_inplace_plan.h) through the C ABI.
extern "C" int dsx_inplace_plan(const dsx_plan_seg_t* segs, uint64_t nsegs, const uint64_t* ends,
                                uint64_t n, const uint8_t* keep, uint64_t have_len,
                                uint64_t new_len, uint64_t skew, uint64_t tile, uint64_t window,
                                uint64_t stash_cap, uint32_t flags, dsx_inplace_launch_t* launches,
                                uint64_t launch_cap, dsx_plan_seg_t* out_segs, uint64_t seg_cap,
                                dsx_inplace_totals_t* totals) {
  if (!totals || (launch_cap && !launches) || (seg_cap && !out_segs)) return DSX_E_INVAL;
  *totals = dsx_inplace_totals_t{};
  try {
    dsx_host::InplacePlan plan;
    const int rc = dsx_host::inplace_plan(segs, nsegs, ends, n, keep, have_len, new_len, skew, tile,
                                          window, stash_cap, flags, &plan);
    if (rc == DSX_E_INVAL) return rc;
    *totals = plan.totals;
    if (rc) return rc;
    if (plan.launches.size() > launch_cap || plan.segs.size() > seg_cap) return DSX_E_CAPACITY;
    std::copy(plan.launches.begin(), plan.launches.end(), launches);
    std::copy(plan.segs.begin(), plan.segs.end(), out_segs);
    return DSX_OK;
  } catch (const std::bad_alloc&) {
    return DSX_E_NOMEM;
  }
}
