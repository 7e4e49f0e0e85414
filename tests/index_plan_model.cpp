// index_plan_model.cpp -- the plans of the file pipeline on the CPU.
//
// A stand-alone host program over desync_amd/csrc/dsx_index_plan.h, the header
// run_index and run_ids (dsx_index.cpp) take their windows, pieces, shares and
// cuts from.  tests/test_host_logic.py builds it with
// -fsanitize=address,undefined and runs it: index_schedule over file lengths,
// slots, windows and thread counts, ids_schedule over seeded chunk lists (ends
// only, no bytes, so a list may describe several GiB).  Every chunk of the
// last window must be hashed by exactly one of the GPU's shares, the host and
// the digest after the read.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dsx_index_plan.h"

using namespace dsx_host;

static int failures = 0;
#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond)) {                                     \
      if (++failures <= 40) {                          \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                      \
        std::printf("\n");                             \
      }                                                \
    }                                                  \
  } while (0)
typedef unsigned long long ull;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr uint64_t KiB = 1ull << 10, MiB = 1ull << 20, GiB = 1ull << 30;
constexpr uint64_t kMax = 256 * KiB;
static const uint64_t kSlots[] = {256 * KiB, 1 * MiB, 32 * MiB, 288 * MiB, 1 * GiB};
static const uint64_t kWindows[] = {1 * MiB, 80 * MiB, 1 * GiB};
static const int kThreads[] = {1, 12, 28};
static const int64_t kHostTails[] = {-1, 0, 40000};

// one cut per segment: the host takes exactly what the GPU skips
static bool one_cut(uint64_t feed, uint64_t skip, uint64_t max_chunk) {
  return feed == skip || (feed >= max_chunk && skip == 0);
}

// ---- run_index ---------------------------------------------------------------
static uint64_t n_index = 0, n_index_shares = 0, n_index_dropped = 0;
static void check_index(uint64_t len, uint64_t slot, uint64_t window, int threads, int64_t host_tail) {
  const bool feeds = host_tail != 0;
  const IndexGeom g(len, kMax, slot, window, feeds);
  const IndexSchedule s = index_schedule(g, len, kMax, threads, host_tail, feeds);
  const ull l = len, sl = slot, wi = window;
  ++n_index;
  CHECK(g.pre >= kMax + 64 && g.pre % 128 == 0 && g.piece % 4096 == 0 && g.piece <= ((std::max<uint64_t>(slot, 4096) + 4095) & ~4095ull),
        "len %llu slot %llu: pre %llu piece %llu", l, sl, (ull)g.pre, (ull)g.piece);
  CHECK(g.W % g.piece == 0 && g.W >= g.piece && g.nwin >= 1 && (g.nwin - 1) * g.W < len && g.nwin * g.W >= len,
        "len %llu slot %llu window %llu: W %llu x %llu", l, sl, wi, (ull)g.W, (ull)g.nwin);
  CHECK(g.nwin == 1 || g.W >= 2 * g.pre, "len %llu: windows of %llu keep %llu", l, (ull)g.W, (ull)g.pre);
  // the pieces tile the file, none crossing a window's end; the scan points
  // are piece ends that rise to len and include every window's end
  const PieceMap pm(len, g.piece, g.fine_from, g.fine);
  uint64_t pos = 0;
  size_t sp = 0;
  for (uint64_t k = 0; k < pm.np; ++k) {
    CHECK(pm.off(k) == pos && pm.size(k) > 0 && pm.size(k) <= g.piece, "len %llu: piece %llu", l, (ull)k);
    CHECK(pos / g.W == (pos + pm.size(k) - 1) / g.W, "len %llu: piece %llu crosses a window", l, (ull)k);
    pos += pm.size(k);
    if (sp < s.scan.size() && s.scan[sp] == pos) ++sp;
    CHECK(sp > 0 ? pos - s.scan[sp - 1] < std::max(2 * g.piece, kScanStep + g.piece) : pos < kScanStep + g.piece,
          "len %llu: no scan point for %llu bytes", l, (ull)pos);
    if (pos % g.W == 0 || pos == len) CHECK(sp > 0 && s.scan[sp - 1] == pos, "len %llu: window end %llu unscanned", l, (ull)pos);
  }
  CHECK(pos == len && sp == s.scan.size() && !s.scan.empty() && s.scan.back() == len,
        "len %llu slot %llu: %zu of %zu scan points are piece ends", l, sl, sp, s.scan.size());
  // the segments tile the last window, one cut each
  CHECK(s.last_ws == (g.nwin - 1) * g.W && s.side0 == (g.nwin > 1 ? 1u : 0u), "len %llu: last window", l);
  pos = s.last_ws;
  for (const ShareSeg& q : s.segs) {
    CHECK(q.from == pos && q.to > q.from, "len %llu slot %llu: segment [%llu, %llu) after %llu", l, sl,
          (ull)q.from, (ull)q.to, (ull)pos);
    CHECK(one_cut(q.feed_cut, q.skip_above, kMax), "len %llu slot %llu: host above %llu, GPU skips above %llu", l,
          sl, (ull)q.feed_cut, (ull)q.skip_above);
    pos = q.to;
  }
  CHECK(pos == len && s.segs.size() == s.fired.size() + 1, "len %llu: segments end at %llu", l, (ull)pos);
  CHECK(feeds == (s.segs.back().feed_cut != UINT64_MAX), "len %llu: feeder %d", l, (int)feeds);
  // the fired shares: in order, at scan points below len at or after their
  // point, one side stream each; a dropped one leaves no cut behind
  CHECK(s.fired.size() + s.side0 <= (size_t)kIdxSide && s.fire.size() == s.mids.size(), "len %llu: sides", l);
  size_t j = 0;
  for (size_t k = 0; k < s.mids.size(); ++k) {
    if (!s.fire[k]) continue;
    CHECK(j < s.fired.size() && s.fired[j].at == s.fire[k] && s.fired[j].cut == s.mids[k].cut && j == k,
          "len %llu slot %llu: share %zu", l, sl, k);
    CHECK(s.fire[k] >= s.mids[k].at && s.fire[k] < len && s.fire[k] > s.last_ws &&
              std::find(s.scan.begin(), s.scan.end(), s.fire[k]) != s.scan.end(),
          "len %llu slot %llu: share %zu due at %llu fires at %llu", l, sl, k, (ull)s.mids[k].at, (ull)s.fire[k]);
    if (j < s.fired.size()) {
      CHECK(s.segs[j].to == s.fire[k] && s.segs[j].feed_cut == s.mids[k].cut, "len %llu: segment %zu", l, j);
      CHECK(j == 0 || s.fired[j - 1].at < s.fired[j].at, "len %llu: shares out of order", l);
    }
    ++j;
  }
  CHECK(j == s.fired.size(), "len %llu slot %llu: %zu shares fired, %zu listed", l, sl, j, s.fired.size());
  CHECK(s.segs.back().feed_cut == (feeds ? s.fcut_end : UINT64_MAX) && (!s.fired.empty() || s.fcut_end == s.fcut),
        "len %llu: the last cut", l);
  n_index_shares += !s.fired.empty();
  n_index_dropped += j < s.mids.size();
}

// ---- run_ids -----------------------------------------------------------------
struct List {
  uint64_t start;
  std::vector<uint64_t> ends;
};
// chunks of lo..hi bytes (about `zeros` in 64 of no bytes) up to `total` bytes
static List make_list(uint64_t start, uint64_t total, uint64_t lo, uint64_t hi, unsigned zeros = 0) {
  List li{start, {}};
  for (uint64_t pos = start; pos - start < total;) {
    if (zeros && rnd() % 64 < zeros) {
      li.ends.push_back(pos);
      continue;
    }
    // (skewed to the short side, like a content-defined chunker's)
    const uint64_t r = rnd() % 1024, len = lo + (hi - lo) * r * r / (1023 * 1023);
    pos += std::min(len, total - (pos - start));
    li.ends.push_back(pos);
  }
  return li;
}

static uint64_t n_ids = 0, n_ids_shares = 0, n_ids_low_cut = 0;
static void check_ids(const List& li, uint64_t slot, uint64_t window, int threads, int64_t host_tail, bool tail_on,
                      double host_ns) {
  const uint64_t n = li.ends.size(), start = li.start;
  const uint64_t* ends = li.ends.data();
  const IdsSchedule s = ids_schedule(start, ends, n, slot, window, threads, host_tail, kIdxSide, tail_on, host_ns);
  const WindowGeom& g = s.g;
  const ull nn = n, sl = slot, wi = window;
  ++n_ids;
  auto len_of = [&](uint64_t i) { return ends[i] - (i ? ends[i - 1] : start); };
  uint64_t maxc = 0;
  for (uint64_t i = 0; i < n; ++i) maxc = std::max(maxc, len_of(i));
  CHECK(s.L == (n ? ends[n - 1] - start : 0) && s.maxc == maxc, "n %llu: L %llu maxc %llu", nn, (ull)s.L, (ull)s.maxc);
  CHECK(g.pre >= maxc && g.pre % 128 == 0 && g.piece >= 4096 && g.piece % 4096 == 0 && g.W % g.piece == 0 &&
            g.W >= g.piece && g.nwin >= 1 && g.nwin * g.W >= s.L && (g.nwin == 1 || (g.nwin - 1) * g.W < s.L),
        "n %llu slot %llu window %llu: pre %llu piece %llu W %llu x %llu", nn, sl, wi, (ull)g.pre, (ull)g.piece,
        (ull)g.W, (ull)g.nwin);
  CHECK(g.nwin == 1 || g.W >= 2 * g.pre, "n %llu: windows of %llu keep %llu", nn, (ull)g.W, (ull)g.pre);
  // the windows' ranges tile [0, n); every chunk ends in its window and starts
  // inside the bytes the window holds
  CHECK(s.win_i1.size() == g.nwin && s.win_i1.back() == n, "n %llu: %zu window ranges", nn, s.win_i1.size());
  for (uint64_t w = 0, i = 0; w < g.nwin && w < s.win_i1.size(); ++w) {
    const uint64_t ws = w * g.W, we = std::min(s.L, ws + g.W);
    CHECK(s.win_i1[w] >= i && s.win_i1[w] <= n, "n %llu: window %llu ends at chunk %llu", nn, (ull)w, (ull)s.win_i1[w]);
    if (w + 1 == g.nwin) CHECK(i == s.i_last && s.last_ws == ws, "n %llu: the last window starts at chunk %llu", nn, (ull)i);
    for (; i < s.win_i1[w] && i < n; ++i) {
      const uint64_t e = ends[i] - start, b = e - len_of(i);
      CHECK((e > ws || w == 0) && e <= we, "n %llu: chunk %llu ends at %llu in window %llu", nn, (ull)i, (ull)e, (ull)w);
      CHECK(b + g.pre >= ws, "n %llu: chunk %llu starts at %llu, window %llu keeps %llu", nn, (ull)i, (ull)b, (ull)w, (ull)g.pre);
    }
    if (s.win_i1[w] < n) CHECK(ends[s.win_i1[w]] - start > we, "n %llu: window %llu leaves a chunk", nn, (ull)w);
  }
  // the shares: landed points rise in whole pieces below L (two may share a
  // piece end of a large slot: the later one then has no chunks), their chunks
  // end by them
  CHECK(s.shares.size() <= (size_t)kIdxSide && s.segs.size() == s.shares.size() + 1, "n %llu: %zu shares", nn, s.shares.size());
  CHECK(s.shares.empty() || (tail_on && host_tail < 0), "n %llu: shares without the auto host tail", nn);
  uint64_t from = s.i_last;
  for (size_t k = 0; k < s.shares.size() && k + 1 < s.segs.size(); ++k) {
    const IdShare& sh = s.shares[k];
    CHECK(sh.landed % g.piece == 0 && sh.landed < s.L && sh.landed > s.last_ws &&
              (k == 0 || sh.landed > s.shares[k - 1].landed || (sh.landed == s.shares[k - 1].landed && sh.i1 == from)),
          "n %llu slot %llu: share %zu lands at %llu", nn, sl, k, (ull)sh.landed);
    CHECK(sh.i1 >= from && sh.i1 <= n && s.segs[k].i_from == from && s.segs[k].i_to == sh.i1 && s.segs[k].feed_cut == sh.cut,
          "n %llu: share %zu's segment", nn, k);
    for (uint64_t i = from; i < sh.i1 && i < n; ++i)
      CHECK(ends[i] - start <= sh.landed, "n %llu: chunk %llu of share %zu ends after %llu", nn, (ull)i, k, (ull)sh.landed);
    from = sh.i1;
  }
  CHECK(s.segs.back().i_from == from && s.segs.back().i_to == n, "n %llu: the last segment", nn);
  // one cut per segment, and exactly one party per chunk of the last window
  const uint64_t early = feed_cut_for(host_tail, threads);
  CHECK(s.early_cut == early, "n %llu: early cut %llu", nn, (ull)s.early_cut);
  uint64_t fixed = 0;
  std::vector<uint64_t> last;
  for (size_t j = 0; j < s.segs.size(); ++j) {
    const IdSeg& q = s.segs[j];
    CHECK(tail_on ? one_cut(q.feed_cut, q.skip_above, std::max<uint64_t>(maxc, 1)) : q.feed_cut == UINT64_MAX && q.skip_above == 0,
          "n %llu segment %zu: host above %llu, GPU skips above %llu", nn, j, (ull)q.feed_cut, (ull)q.skip_above);
    for (uint64_t i = q.i_from; i < q.i_to && i < n; ++i) {
      const uint64_t ln = len_of(i);
      const bool host = ln > q.feed_cut, gpu = q.skip_above == 0 || ln <= q.skip_above;
      CHECK(host != gpu, "n %llu: chunk %llu of %llu bytes has %d takers", nn, (ull)i, (ull)ln, (int)host + (int)gpu);
      if (j + 1 < s.segs.size()) fixed += host ? ln : 0;
      else last.push_back(ln);
    }
  }
  const uint64_t end = s.segs.back().feed_cut;
  if (!tail_on) return;
  if (s.shares.empty()) {
    CHECK(end == early && s.end_cut == early, "n %llu: no shares, last cut %llu", nn, (ull)end);
    return;
  }
  // end_cut by brute force: the lowest multiple of 4096 up to early_cut whose
  // host bytes fit the budget, early_cut if none does
  ++n_ids_shares;
  const double budget = 0.75 * (double)s.L / kReadBytesPerNs * threads / host_ns;
  uint64_t want = early;
  for (uint64_t cut = 4096; cut <= early; cut += 4096) {
    uint64_t bytes = fixed;
    for (uint64_t ln : last) bytes += ln > cut ? ln : 0;
    if ((double)bytes <= budget) {
      want = cut;
      break;
    }
  }
  CHECK(end == s.end_cut && end == want && end <= early && (end % 4096 == 0 || end == early),
        "n %llu slot %llu threads %d: end cut %llu, brute force %llu", nn, sl, threads, (ull)end, (ull)want);
  n_ids_low_cut += end < early;
}

int main() {
  // run_index: lengths from 1 B to 5 GiB
  std::vector<uint64_t> lens = {1, 4095, 4096, 8 * MiB, 32 * MiB + 1, 80 * MiB + 4321, 352 * MiB + 4321,
                                640 * MiB + 4321, GiB, GiB + 12345, 3 * GiB - 7, 5 * GiB};
  for (int i = 0; i < 24; ++i) lens.push_back(1 + rnd() % (5 * GiB));
  for (uint64_t len : lens)
    for (uint64_t slot : kSlots)
      for (uint64_t window : kWindows)
        for (int threads : kThreads)
          for (int64_t ht : kHostTails) {
            if (window == MiB && len > 256 * MiB) continue;  // (thousands of windows add nothing)
            check_index(len, slot, window, threads, ht);
            check_index(len, std::max<uint64_t>(4096, len), window, threads, ht);
          }
  // run_ids: 16/64/256 KiB lists of 1-5 GiB, and the awkward ones
  std::vector<List> lists;
  for (uint64_t total : {GiB, GiB + 352 * MiB + 4321, 3 * GiB - 7, 5 * GiB})
    lists.push_back(make_list(total % 4096, total, 16 * KiB, 256 * KiB));
  lists.push_back(make_list(12345, 700 * MiB, 16 * KiB, 256 * KiB, 3));   // a start, empty chunks
  lists.push_back(make_list(0, 9 * MiB + 17, 1, 64 * KiB, 8));            // several 1 MiB windows
  lists.push_back(make_list(777, 6 * MiB, 3 * MiB / 2, 3 * MiB));         // chunks longer than a window
  lists.push_back(make_list(5, 100 * KiB, 100 * KiB, 100 * KiB));         // n = 1
  lists.push_back(List{99, {}});                                          // n = 0
  lists.push_back(List{4096, {4096, 4096, 4096}});                        // no bytes at all
  lists.push_back(List{0, {0, 0, 2 * MiB, 2 * MiB, 2 * MiB + 1}});        // ends at 0, a window's last byte
  for (const List& li : lists)
    for (uint64_t slot : kSlots)
      for (uint64_t window : kWindows)
        for (int threads : kThreads)
          for (int64_t ht : kHostTails)
            for (double host_ns : {0.38, 1.52}) {
              if (window == MiB && !li.ends.empty() && li.ends.back() - li.start > 256 * MiB) continue;
              check_ids(li, slot, window, threads, ht, ht != 0, host_ns);
              if (ht < 0 && host_ns < 1) check_ids(li, slot, window, threads, ht, false, host_ns);  // (SHA-256)
            }
  // (the sweeps reach what they are for)
  CHECK(n_index_shares > 100 && n_index_dropped > 10, "index: %llu with shares, %llu with a dropped one",
        (ull)n_index_shares, (ull)n_index_dropped);
  CHECK(n_ids_shares > 50 && n_ids_low_cut > 10, "ids: %llu with shares, %llu with a lowered end cut",
        (ull)n_ids_shares, (ull)n_ids_low_cut);
  if (failures) {
    std::printf("index plan model: %d failures\n", failures);
    return 1;
  }
  std::printf("index plan model ok: %llu index schedules, %llu ids schedules\n", (ull)n_index, (ull)n_ids);
  return 0;
}
