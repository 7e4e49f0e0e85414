// many_plan_model.cpp -- the plan of a many-blob cut call on the CPU.
//
// A stand-alone host program over desync_amd/csrc/dsx_many_plan.h, the header
// dsx_cut_device_many takes its work items and the batched walk's runs from.
// tests/test_many_host.py builds it with -fsanitize=address,undefined and
// runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsx_many_plan.h"

using dsx_host::ManyItem;
using dsx_host::ManyRun;
using dsx_host::many_plan;
using dsx_host::many_runs;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
    }                                             \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static std::vector<uint64_t> ends_of(const std::vector<uint64_t>& lens) {
  std::vector<uint64_t> e;
  uint64_t at = 0;
  for (uint64_t n : lens) e.push_back(at += n);
  return e;
}

// The properties every plan has; returns the number of items that launch.
static uint64_t check_plan(const std::vector<uint64_t>& lens, uint64_t big, uint64_t group,
                           const char* what) {
  const std::vector<uint64_t> e = ends_of(lens);
  const uint64_t n = e.size();
  const std::vector<ManyItem> items = many_plan(e.data(), n, big, group);
  uint64_t next = 0, launches = 0, at = 0;
  for (size_t k = 0; k < items.size(); ++k) {
    const ManyItem& it = items[k];
    // items tile the blob list in order, and their bytes the buffer
    CHECK(it.b0 == next && it.b1 > it.b0 && it.b1 <= n, "%s: item %zu blobs [%llu, %llu) after %llu",
          what, k, (unsigned long long)it.b0, (unsigned long long)it.b1, (unsigned long long)next);
    next = it.b1;
    CHECK(it.start == at || it.end == it.start, "%s: item %zu starts at %llu, not %llu", what, k,
          (unsigned long long)it.start, (unsigned long long)at);
    if (it.end > it.start) {
      CHECK(it.start == (it.b0 ? e[it.b0 - 1] : 0) && it.end == e[it.b1 - 1],
            "%s: item %zu bytes are not its blobs' bytes", what, k);
      at = it.end;
      ++launches;
    }
    uint64_t nonempty = 0;
    for (uint64_t i = it.b0; i < it.b1; ++i) {
      const uint64_t len = lens[i];
      if (!len) continue;
      ++nonempty;
      if (it.single) {
        CHECK(i == it.big, "%s: single item %zu holds a second blob %llu", what, k, (unsigned long long)i);
        CHECK(len >= big || len > group, "%s: a small blob %llu is single", what, (unsigned long long)i);
      } else {
        CHECK(len < big, "%s: blob %llu of %llu bytes >= big_blob in a group", what,
              (unsigned long long)i, (unsigned long long)len);
      }
    }
    if (it.single) CHECK(nonempty == 1, "%s: single item %zu with %llu blobs", what, k, (unsigned long long)nonempty);
    else CHECK(it.end - it.start <= group, "%s: group %zu of %llu bytes", what, k, (unsigned long long)(it.end - it.start));
    // empty blobs cost nothing: no item of their own unless there is nothing else
    if (nonempty == 0) CHECK(items.size() == 1, "%s: an item of empty blobs only", what);
    // groups are maximal: the next item's first blob would not have fitted
    if (!it.single && k + 1 < items.size() && !items[k + 1].single && it.end > it.start) {
      const ManyItem& nx = items[k + 1];
      uint64_t j = nx.b0;
      while (j < nx.b1 && lens[j] == 0) ++j;
      CHECK(j < nx.b1 && e[j] - it.start > group, "%s: group %zu is not maximal", what, k);
    }
  }
  CHECK(next == n, "%s: the items cover %llu of %llu blobs", what, (unsigned long long)next, (unsigned long long)n);
  CHECK(n == 0 || at == e[n - 1], "%s: the items cover %llu of the bytes", what, (unsigned long long)at);
  return launches;
}

static void check_runs(const std::vector<uint64_t>& lens, uint64_t b0, uint64_t b1, uint64_t span,
                       uint32_t max_blobs) {
  const std::vector<uint64_t> e = ends_of(lens);
  std::vector<ManyRun> runs;
  many_runs(e.data(), b0, b1, span, max_blobs, &runs);
  uint64_t next = b0;
  for (const ManyRun& r : runs) {
    CHECK(r.b0 == next && r.b1 > r.b0, "runs: [%u, %u) after %llu", r.b0, r.b1, (unsigned long long)next);
    next = r.b1;
    CHECK(r.b1 - r.b0 <= max_blobs, "runs: %u blobs", r.b1 - r.b0);
    const uint64_t lo = r.b0 ? e[r.b0 - 1] : 0;
    CHECK(r.b1 - r.b0 == 1 || e[r.b1 - 1] - lo <= span, "runs: [%u, %u) spans %llu", r.b0, r.b1,
          (unsigned long long)(e[r.b1 - 1] - lo));
  }
  CHECK(next == b1, "runs cover up to %llu of %llu", (unsigned long long)next, (unsigned long long)b1);
}

int main() {
  const uint64_t MiB = 1ull << 20;
  // the corners
  CHECK(many_plan(nullptr, 0, 4 * MiB, 8 * MiB).empty(), "no blob: no item");
  CHECK(check_plan({0, 0, 0}, 4 * MiB, 8 * MiB, "all empty") == 0, "all empty: nothing launches");
  CHECK(many_plan(ends_of({0, 0, 0}).data(), 3, 4 * MiB, 8 * MiB).size() == 1, "all empty: one item");
  CHECK(check_plan({5}, 4 * MiB, 8 * MiB, "one small") == 1, "one small blob");
  CHECK(check_plan({0}, 4 * MiB, 8 * MiB, "one empty") == 0, "one empty blob");
  {
    const auto e = ends_of({5 * MiB});
    const auto it = many_plan(e.data(), 1, 4 * MiB, 8 * MiB);
    CHECK(it.size() == 1 && it[0].single && it[0].big == 0, "one big blob is single");
  }
  {  // a blob longer than group_bytes but shorter than big_blob is made single
    const auto e = ends_of({MiB, 3 * MiB, MiB});
    const auto it = many_plan(e.data(), 3, 16 * MiB, 2 * MiB);
    CHECK(it.size() == 3 && !it[0].single && it[1].single && it[1].big == 1 && !it[2].single,
          "a blob over group_bytes");
    check_plan({MiB, 3 * MiB, MiB}, 16 * MiB, 2 * MiB, "over group_bytes");
  }
  {  // a blob of exactly big_blob is single, one byte less is not
    const auto e = ends_of({4 * MiB - 1, 4 * MiB});
    const auto it = many_plan(e.data(), 2, 4 * MiB, 64 * MiB);
    CHECK(it.size() == 2 && !it[0].single && it[1].single, "the big_blob threshold");
  }
  {  // a group of exactly group_bytes, and blob ends on its multiples
    const auto e = ends_of({MiB, MiB, 2 * MiB, MiB, 3 * MiB, 1});
    const auto it = many_plan(e.data(), 6, 64 * MiB, 4 * MiB);
    CHECK(it.size() == 3 && it[0].b1 == 3 && it[0].end == 4 * MiB && it[1].b1 == 5 && it[2].b1 == 6,
          "groups filled to the byte");
  }
  {  // runs of empty blobs join the item they touch
    const auto e = ends_of({0, 0, 7, 0, 9 * MiB, 0, 0, 3, 0});
    const auto it = many_plan(e.data(), 9, 4 * MiB, 8 * MiB);
    CHECK(it.size() == 3 && it[0].b0 == 0 && it[0].b1 == 4 && it[1].single && it[1].big == 4 &&
              it[1].b1 == 7 && it[2].b0 == 7 && it[2].b1 == 9,
          "empty blobs join their neighbours");
    CHECK(check_plan({0, 0, 7, 0, 9 * MiB, 0, 0, 3, 0}, 4 * MiB, 8 * MiB, "empties") == 3, "empties: 3 launches");
  }
  // a seeded sweep
  uint64_t plans = 0;
  for (int round = 0; round < 400; ++round) {
    const uint64_t n = rnd() % 200;
    const uint64_t big = 1 + rnd() % (8 * MiB), group = 1 + rnd() % (16 * MiB);
    std::vector<uint64_t> lens;
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t k = rnd() % 8;
      lens.push_back(k < 2 ? 0 : k < 6 ? rnd() % (256 << 10) : rnd() % (12 * MiB));
    }
    check_plan(lens, big, group, "sweep");
    if (n) {
      const uint64_t b0 = rnd() % n, b1 = b0 + 1 + rnd() % (n - b0);
      check_runs(lens, b0, b1, 1 + rnd() % (2 * MiB), 1 + (uint32_t)(rnd() % 64));
    }
    ++plans;
  }
  if (failures) {
    std::printf("many plan model: %d failures\n", failures);
    return 1;
  }
  std::printf("many plan model ok: %llu sweep plans\n", (unsigned long long)plans);
  return 0;
}
