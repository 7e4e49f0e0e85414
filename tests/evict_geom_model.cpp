// evict_geom_model.cpp -- dsx_evict_geom.h alone, under the host sanitizers:
// the radix descent of dsx_store_evict made of dsx_evict::choose, over seeded
// entries, against a linear walk of the entries sorted by (stamp, entry
// number).  The descent must find the stamp of the last entry of the shortest
// prefix that meets both needs, the entries and bytes below that stamp, and the
// needs left inside its class; it must say "not reached" exactly when all
// entries together do not meet them.  A difference is a non-zero exit.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "dsx_evict_geom.h"

namespace {

struct Entry {
  uint64_t stamp, size;
};

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Result {
  bool reached;
  uint64_t cutoff, below_count, below_bytes, need_chunks, need_bytes;
};

// the descent as dsx_store_evict runs it: one histogram and one choice per byte of the clock
Result descend(const std::vector<Entry>& es, uint64_t clock, uint64_t nc, uint64_t nb) {
  Result r{true, 0, 0, 0, nc, nb};
  const int passes = dsx_evict::passes_of(clock);
  uint64_t prefix = 0;
  for (int p = 0; p < passes; ++p) {
    const int level = passes - 1 - p;
    std::vector<dsx_evict::Pair> h(dsx_evict::kBuckets, dsx_evict::Pair{0, 0});
    for (const Entry& e : es) {
      const uint64_t above = level >= 7 ? 0 : e.stamp >> (8 * (level + 1));
      if (above != prefix) continue;
      dsx_evict::Pair& b = h[(e.stamp >> (8 * level)) & 255];
      b.count += 1;
      b.bytes += e.size;
    }
    const dsx_evict::Choice c = dsx_evict::choose(h.data(), r.need_chunks, r.need_bytes);
    if (c.bucket < 0) {
      if (p != 0) {
        printf("not reached below the top pass\n");
        exit(1);
      }
      r.reached = false;
      return r;
    }
    prefix = (prefix << 8) | (uint64_t)c.bucket;
    r.need_chunks = c.need_chunks;
    r.need_bytes = c.need_bytes;
    r.below_count += c.below_count;
    r.below_bytes += c.below_bytes;
  }
  r.cutoff = prefix;
  return r;
}

// the definition: walk the entries in ascending stamp until both needs are met
Result walk(std::vector<Entry> es, uint64_t nc, uint64_t nb) {
  std::stable_sort(es.begin(), es.end(), [](const Entry& a, const Entry& b) { return a.stamp < b.stamp; });
  uint64_t count = 0, bytes = 0;
  size_t k = 0;
  while (k < es.size() && !(count >= nc && bytes >= nb)) {
    count += 1;
    bytes += es[k].size;
    ++k;
  }
  Result r{count >= nc && bytes >= nb, 0, 0, 0, 0, 0};
  if (!r.reached) return r;
  r.cutoff = es[k - 1].stamp;  // (k > 0: one need is above 0)
  for (const Entry& e : es)
    if (e.stamp < r.cutoff) r.below_count += 1, r.below_bytes += e.size;
  r.need_chunks = nc > r.below_count ? nc - r.below_count : 0;
  r.need_bytes = nb > r.below_bytes ? nb - r.below_bytes : 0;
  return r;
}

}  // namespace

int main() {
  static const uint64_t kClocks[] = {1, 3, 255, 256, 0x1FF, 0xFFFF, 0x10000, 0x100000007ull,
                                     0xFFFFFFFFFFull, 0xFFFFFFFFFFFFFFF0ull, 0xFFFFFFFFFFFFFFFFull};
  static const int kWant[] = {1, 1, 1, 2, 2, 2, 3, 5, 5, 8, 8};
  for (size_t i = 0; i < sizeof kClocks / sizeof *kClocks; ++i)
    if (dsx_evict::passes_of(kClocks[i]) != kWant[i]) {
      printf("passes_of(%llx) = %d, want %d\n", (unsigned long long)kClocks[i], dsx_evict::passes_of(kClocks[i]),
             kWant[i]);
      return 1;
    }
  if (dsx_evict::passes_of(0) != 1) return 1;
  long cases = 0, unreached = 0;
  for (int round = 0; round < 4000; ++round) {
    const uint64_t clock = kClocks[rnd() % (sizeof kClocks / sizeof *kClocks)];
    const size_t n = rnd() % 300;
    const uint64_t classes = 1 + rnd() % 6;  // few distinct stamps: big classes, or many
    std::vector<uint64_t> stamps;
    for (uint64_t k = 0; k < classes; ++k) stamps.push_back(clock == UINT64_MAX ? rnd() : rnd() % (clock + 1));
    stamps.push_back(clock);
    stamps.push_back(0);
    std::vector<Entry> es(n);
    uint64_t all_bytes = 0;
    for (Entry& e : es) {
      e.stamp = rnd() % 3 ? stamps[rnd() % stamps.size()] : (clock == UINT64_MAX ? rnd() : rnd() % (clock + 1));
      e.size = rnd() % 4 ? rnd() % 5000 : 0;
      all_bytes += e.size;
    }
    for (int q = 0; q < 6; ++q) {
      uint64_t nc = rnd() % 3 ? rnd() % (n + 2) : 0;
      uint64_t nb = rnd() % 3 ? rnd() % (all_bytes + 2) : 0;
      if (!nc && !nb) nc = 1;  // (the empty prefix never reaches the descent)
      const Result a = descend(es, clock, nc, nb), b = walk(es, nc, nb);
      ++cases;
      unreached += !b.reached;
      const bool same = a.reached == b.reached &&
                        (!a.reached || (a.cutoff == b.cutoff && a.below_count == b.below_count &&
                                        a.below_bytes == b.below_bytes && a.need_chunks == b.need_chunks &&
                                        a.need_bytes == b.need_bytes));
      if (!same) {
        printf("round %d query %d: n %zu clock %llx needs %llu chunks %llu bytes: descent %d %llx %llu %llu %llu %llu, "
               "walk %d %llx %llu %llu %llu %llu\n", round, q, n, (unsigned long long)clock, (unsigned long long)nc,
               (unsigned long long)nb, a.reached, (unsigned long long)a.cutoff, (unsigned long long)a.below_count,
               (unsigned long long)a.below_bytes, (unsigned long long)a.need_chunks, (unsigned long long)a.need_bytes,
               b.reached, (unsigned long long)b.cutoff, (unsigned long long)b.below_count,
               (unsigned long long)b.below_bytes, (unsigned long long)b.need_chunks, (unsigned long long)b.need_bytes);
        return 1;
      }
      if (a.reached && !a.need_chunks && !a.need_bytes) {
        printf("round %d: no need left inside the class\n", round);
        return 1;
      }
    }
  }
  printf("evict geom model ok: %ld cases, %ld not reached\n", cases, unreached);
  return 0;
}
