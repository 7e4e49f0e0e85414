// known_model.cpp -- the arithmetic of dsx_chunk_ids_known on the CPU.
//
// A stand-alone host program over desync_amd/csrc/dsx_known_geom.h, the header
// the sketch, probe and compare kernels take their fingerprint windows and
// their tiles from.  tests/test_known_host.py builds it with
// -fsanitize=address,undefined and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsx_known_geom.h"

using namespace dsx_known;

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

// The windows lie inside the chunk, are 96 bytes at most, and the fingerprint
// reads exactly them: a buffer of exactly `size` bytes (the sanitizer sees any
// byte read outside it), and a flip changes the fingerprint exactly inside a
// window.
static void check_size(uint64_t size) {
  const Windows w = known_windows(size);
  uint64_t total = 0;
  CHECK(w.n == (size >= 96 ? 3u : 2u), "size %llu: %u windows", (unsigned long long)size, w.n);
  for (uint32_t k = 0; k < w.n; ++k) {
    CHECK(w.off[k] <= size && w.len[k] <= size - w.off[k], "size %llu: window %u leaves the chunk",
          (unsigned long long)size, k);
    CHECK(w.len[k] == (size < 32 ? size : 32), "size %llu: window %u has %u bytes",
          (unsigned long long)size, k, w.len[k]);
    total += w.len[k];
  }
  CHECK(total <= 96, "size %llu: %llu window bytes", (unsigned long long)size, (unsigned long long)total);
  CHECK(w.off[0] == 0 && w.off[1] + w.len[1] == size, "size %llu: first and last window",
        (unsigned long long)size);
  if (w.n == 3)
    CHECK(w.off[2] == size / 2 - 16, "size %llu: middle window at %llu", (unsigned long long)size,
          (unsigned long long)w.off[2]);
  std::vector<uint8_t> buf(size);
  for (auto& b : buf) b = (uint8_t)rnd();
  const uint64_t fp = fingerprint(buf.data(), size);
  CHECK(fp == fingerprint(buf.data(), size), "size %llu: the fingerprint is a function",
        (unsigned long long)size);
  std::vector<uint64_t> at = {0, 1, 15, 16, 31, 32, 33, 40, size / 2 - 17, size / 2 - 16, size / 2,
                              size / 2 + 15, size / 2 + 16, size - 33, size - 32, size - 1};
  for (uint64_t p : at) {
    if (p >= size) continue;
    bool inside = false;
    for (uint32_t k = 0; k < w.n; ++k) inside = inside || (p >= w.off[k] && p - w.off[k] < w.len[k]);
    buf[p] ^= 0x40;
    CHECK((fingerprint(buf.data(), size) != fp) == inside, "size %llu: a flip at %llu, %s a window",
          (unsigned long long)size, (unsigned long long)p, inside ? "inside" : "outside");
    buf[p] ^= 0x40;
  }
}

struct HostBeg {
  const std::vector<uint64_t>* beg;
  uint64_t operator()(uint64_t j) const { return (*beg)[j]; }
};

// The tiles partition the pair bytes exactly: every byte of every pair is taken
// by one tile, in order, and no tile takes more than kTile bytes.
static void check_tiles(const std::vector<uint32_t>& cnt, const std::vector<uint64_t>& size,
                        uint64_t tile, const char* what) {
  const uint64_t n = cnt.size();
  std::vector<uint64_t> beg(n);
  uint64_t total = 0;
  for (uint64_t j = 0; j < n; ++j) beg[j] = total, total += (uint64_t)cnt[j] * size[j];
  // next[j][t]: the next byte of pair t of chunk j some tile must take
  std::vector<std::vector<uint64_t>> next(n);
  for (uint64_t j = 0; j < n; ++j) next[j].assign(cnt[j], 0);
  const HostBeg hb{&beg};
  for (uint64_t lo = 0; lo < total; lo += tile) {
    const uint64_t hi = lo + tile < total ? lo + tile : total;
    uint64_t taken = 0;
    uint64_t j = chunk_at(hb, n, lo);
    CHECK(beg[j] <= lo && lo < beg[j] + (uint64_t)cnt[j] * size[j], "%s: tile at %llu starts in chunk %llu",
          what, (unsigned long long)lo, (unsigned long long)j);
    for (; j < n; ++j) {
      if (beg[j] >= hi) break;
      if (!cnt[j]) continue;
      const Part p = part_of(beg[j], cnt[j], size[j], lo, hi);
      for (uint32_t t = p.t0; t <= p.t1 && t < cnt[j]; ++t) {
        uint64_t a, z;
        pair_bytes(p, t, size[j], &a, &z);
        CHECK(a < z && z <= size[j], "%s: pair bytes [%llu, %llu) of %llu", what,
              (unsigned long long)a, (unsigned long long)z, (unsigned long long)size[j]);
        CHECK(next[j][t] == a, "%s: chunk %llu pair %u continues at %llu, not %llu", what,
              (unsigned long long)j, t, (unsigned long long)a, (unsigned long long)next[j][t]);
        CHECK(beg[j] + t * size[j] + a >= lo && beg[j] + t * size[j] + z <= hi, "%s: outside the tile", what);
        next[j][t] = z;
        taken += z - a;
      }
    }
    CHECK(taken == hi - lo, "%s: tile at %llu takes %llu of %llu bytes", what, (unsigned long long)lo,
          (unsigned long long)taken, (unsigned long long)(hi - lo));
  }
  for (uint64_t j = 0; j < n; ++j)
    for (uint32_t t = 0; t < cnt[j]; ++t)
      CHECK(next[j][t] == size[j], "%s: chunk %llu pair %u compared up to %llu of %llu", what,
            (unsigned long long)j, t, (unsigned long long)next[j][t], (unsigned long long)size[j]);
}

int main() {
  uint64_t sizes = 0;
  for (uint64_t s = 0; s <= 300; ++s, ++sizes) check_size(s);
  for (uint64_t m = 1; m <= 3; ++m)
    for (uint64_t s = m * kTile - 2; s <= m * kTile + 18; ++s, ++sizes) check_size(s);

  int lists = 0;
  // the shapes of the GPU test: tiny chunks, chunks around the tile, empty ones
  check_tiles({1, 4, 0, 2, 1}, {kTile - 1, kTile, 5, kTile + 1, 2 * kTile + 17}, kTile, "around the tile");
  check_tiles({0, 0, 3, 0}, {9, 0, 1, 7}, kTile, "one byte");
  check_tiles({2, 1, 4}, {0, 0, 0}, kTile, "no bytes");
  check_tiles({}, {}, kTile, "no chunks");
  lists += 4;
  for (int round = 0; round < 300; ++round, ++lists) {
    const uint64_t tile = round % 3 == 0 ? 64 : kTile;  // (a small tile: many tiles per pair)
    const uint64_t n = rnd() % 200;
    std::vector<uint32_t> cnt(n);
    std::vector<uint64_t> size(n);
    for (uint64_t j = 0; j < n; ++j) {
      cnt[j] = (uint32_t)(rnd() % (kTries + 1));
      const uint64_t r = rnd() % 10;
      size[j] = r == 0 ? 0 : r < 6 ? rnd() % 200 : r < 9 ? rnd() % (3 * tile) : tile * (1 + rnd() % 3);
    }
    check_tiles(cnt, size, tile, "random");
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("known model ok: %llu sizes, %d pair lists\n", (unsigned long long)sizes, lists);
  return 0;
}
