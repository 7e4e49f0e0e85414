// CPU model of scanl_kernel<..., ROTF> (desync_amd/csrc/dsx_rotframe.h), built
// and run by tests/test_rotframe_model.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -Iinclude -Idesync_amd/csrc tests/rotframe_model.cpp
//
// 64 lanes roll the hash in the rotating frame over a 48-byte warm-up and
// NBYTES more bytes with the kernel's own schedule (subgroups of 8 bytes, the
// lookups of subgroup j+1 issued before subgroup j is hashed, every lookup
// landing in ring register i mod 64), taking table offsets, rotations and
// phase registers from dsx_rotframe.h.  At every position the un-rotated x
// must be the complement of the direct Buzhash of the last 48 bytes (MODE 2
// keeps x = ~h).  Lanes 0..31 warm up on random bytes, lanes 32..63 on a
// zero window (the kernel's lanes 1..63).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dsx_buzhash_table.h"
#include "dsx_rotframe.h"

namespace rf = dsx::rotframe;

static const uint32_t kT[256] = DSX_BUZHASH_TABLE_INIT;

// v_perm_b32 D = perm(S0, S1, sel): selector bytes 0..3 pick S1's bytes,
// 4..7 S0's, 0x0C a zero byte (the only selectors the kernel uses)
static uint32_t v_perm(uint32_t s0, uint32_t s1, uint32_t sel) {
  uint32_t out = 0;
  for (int b = 0; b < 4; ++b) {
    const uint32_t s = (sel >> (8 * b)) & 0xFFu;
    uint32_t byte = 0;
    if (s < 4) byte = (s1 >> (8 * s)) & 0xFFu;
    else if (s < 8) byte = (s0 >> (8 * (s - 4))) & 0xFFu;
    else if (s != 0x0C) abort();
    out |= byte << (8 * b);
  }
  return out;
}

static uint32_t direct_buzhash(const uint8_t* win) {  // win[0] oldest .. win[47] newest
  uint32_t h = 0;
  for (int j = 0; j < rf::kWindow; ++j) h ^= rf::rotl32(kT[win[j]], (uint32_t)(rf::kWindow - 1 - j));
  return h;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

int main() {
  constexpr int NBYTES = 2 * 384 + 96;  // two trips, the 48-byte extension and 48 more
  static_assert(NBYTES % 8 == 0, "whole subgroups");
  long bad = 0;

  // the LDS table image
  std::vector<uint32_t> lds(rf::kTableBytes / 4);
  std::vector<int> written(lds.size(), 0);
  for (uint32_t v = 0; v < 256; ++v)
    for (uint32_t k = 0; k < (uint32_t)rf::kSlots; ++k) {
      const uint32_t off = rf::table_offset(v, k);
      if (off % 4 || off / 4 >= lds.size()) { printf("table offset out of range\n"); return 1; }
      lds[off / 4] = rf::table_value(kT[v], k);
      ++written[off / 4];
    }
  for (int wv : written) bad += wv != 1;
  if (bad) { printf("table image not covered exactly once\n"); return 1; }

  // each phase: the 64 lanes read 64 distinct banks whatever their bytes are,
  // and v_perm_b32 with lookup_sel builds table_offset(byte, slot)
  for (uint32_t f = 0; f < (uint32_t)rf::kPhases; ++f) {
    uint64_t banks = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t pr = rf::phase_reg(lane, f), w = rng();
      for (int k = 0; k < 4; ++k) {
        const uint32_t off = v_perm(w, pr, rf::lookup_sel(k));
        const uint32_t byte = (w >> (8 * k)) & 0xFFu;
        if (off != rf::lookup_offset(w, pr, k) || off != rf::table_offset(byte, rf::slot_of(lane, f))) {
          printf("phase %u lane %u byte %d: offset %u\n", f, lane, k, off);
          ++bad;
        }
        if (k == 0) banks |= 1ull << ((off / 4) % 64);
      }
      if (rf::phase_reg_rot(pr) != ((lane - f) & 31u)) ++bad;
    }
    if (banks != ~0ull) {
      printf("phase %u: bank conflict (%016llx)\n", f, (unsigned long long)banks);
      ++bad;
    }
  }

  for (uint32_t lane = 0; lane < 64; ++lane) {
    uint32_t ph[rf::kPhases];
    for (int f = 0; f < rf::kPhases; ++f) ph[f] = rf::phase_reg(lane, (uint32_t)f);
    // bytes[48 + i] is stream position i; the warm-up is positions -48 .. -1
    std::vector<uint8_t> bytes(rf::kWindow + NBYTES);
    for (size_t j = 0; j < bytes.size(); ++j)
      bytes[j] = (lane >= 32 && j < (size_t)rf::kWindow) ? 0 : (uint8_t)rng();
    auto word_of = [&](int i) {  // the dword that holds position i, as the kernel's w[]
      uint32_t w;
      memcpy(&w, &bytes[(size_t)((rf::kWindow + i) & ~3)], 4);
      return w;
    };
    std::vector<uint32_t> ring((size_t)rf::kRing, 0xDEADBEEFu);  // never read before written
    uint32_t g = ~0u;
    auto issue = [&](int i0) {  // the 8 lookups of the subgroup at position i0
      for (int q = 0; q < 8; ++q) {
        const int i = i0 + q;
        const uint32_t off = v_perm(word_of(i), ph[rf::phase_of(i)], rf::lookup_sel((rf::kWindow + i) & 3));
        ring[(size_t)rf::ring_in(i)] = lds[off / 4];
      }
    };
    issue(-rf::kWindow);
    for (int i0 = -rf::kWindow; i0 < NBYTES; i0 += 8) {
      if (i0 + 8 < NBYTES) issue(i0 + 8);
      for (int q = 0; q < 8; ++q) {
        const int i = i0 + q;
        if (i < 0) {
          g ^= ring[(size_t)rf::ring_in(i)];  // warm-up: nothing leaves the window yet
          continue;
        }
        g ^= ring[(size_t)rf::ring_in(i)] ^ ring[(size_t)rf::ring_out(i)];
        const uint32_t x = rf::unrotate(g, ph[rf::phase_of(i)]);
        const uint32_t want = ~direct_buzhash(&bytes[(size_t)(i + 1)]);  // bytes of i-47 .. i
        if (x != want) {
          if (bad < 10) printf("lane %u position %d: x %08x, want %08x\n", lane, i, x, want);
          ++bad;
        }
      }
    }
  }
  if (bad) {
    printf("%ld mismatches\n", bad);
    return 1;
  }
  printf("rotframe model ok: 64 lanes x %d positions, 32 phases conflict-free\n", NBYTES);
  return 0;
}
