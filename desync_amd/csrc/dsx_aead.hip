// dsx_aead.hip -- the AEAD store converter of encrypt.go on the GPU:
// XChaCha20-Poly1305, Go's chacha20poly1305.NewX(key).Seal(out, nonce, in, nil)
// for every chunk of a resident blob at once.  A record is
// nonce(24) || ciphertext || tag(16).
//
// Launches:
//   setup   one lane per record: HChaCha20 -> subkey, ChaCha20 block 0 -> the
//           one-time key (r clamped, s), r^2, r^3, r^4 and r^1024; seal writes
//           the nonce into the record.
//   main    work divided by plaintext bytes: a workgroup owns the 64-byte cipher
//           blocks whose first byte lies in its tile of kAeadTile bytes, of
//           however many chunks.  A lane takes every 256th block of a piece
//           (chunk x tile; a piece of up to 64 blocks is one wave's), xors the
//           keystream and folds the ciphertext it holds in registers into a
//           Poly1305 sum by Horner's rule with r^1024, then
//           weights the sum by r^(blocks to the chunk's end), computed by
//           square-and-multiply.  A wave adds its lanes' terms and writes them
//           to the slot (chunk + tile, wave): no lane waits for another one, and
//           no slot depends on the order of arrival.
//   finish  one wave per record adds the record's slots, the length block and
//           s, and writes the tag (seal) or compares it (open).
//   scrub   open only, if a record failed: zero-fills its plaintext.
// All arithmetic is integer; nothing is accumulated with atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <string>
#include <unordered_set>
#include <vector>

#include "dsx_callargs.h"
#include "dsx_engine.h"

namespace dsx {

typedef unsigned long long u64;
constexpr int kAeadThreads = 64 * kAeadWaves;
constexpr u64 kTile = kAeadTile;
constexpr u64 kAeadMaxChunk = (1ull << 38) - 64;  // ChaCha20's 32-bit block counter starts at 1
constexpr u64 kNonce = 24, kOverhead = 40;        // (dsx.h's names for them are checked below)
constexpr u64 kShort = ~0ull;                     // offs[i]: a record too short to hold nonce and tag
static_assert(kTile % (64 * kAeadThreads) == 0, "a tile is whole passes of the workgroup");
static_assert(kTile == DSX_AEAD_TILE && kNonce == DSX_AEAD_NONCE && kOverhead == DSX_AEAD_OVERHEAD,
              "dsx.h names the tile and the record's overhead");

enum { kSeal = 0, kOpen = 1, kMac = 2 };

typedef uint32_t a4u __attribute__((ext_vector_type(4)));
typedef a4u a4u_unaligned __attribute__((aligned(1)));
#define DSX_AGLOBAL __attribute__((address_space(1)))

struct AeadArgs {
  const u64* ends;     // plaintext chunk ends (device); chunk i is [ends[i-1], ends[i]), ends[-1] = start
  u64 start, n, total; // total = ends[n-1] - start
  const u64* offs;     // record offsets, or null: record i at (ends[i-1] - start) + 40 i
  uint8_t* pt;         // plaintext base: byte x of the ends' coordinates is pt[x]
  uint8_t* rec;        // record base
  u64 skip;            // bytes of a record in front of its ciphertext (24; selftest: 0)
  uint32_t* rctx;
  uint32_t* slots;
  uint8_t* flag;
  const uint8_t* key;
  const uint8_t* nonces;
};

// ---- Poly1305 in five 26-bit limbs ---------------------------------------------------
struct Fe {
  uint32_t v[5];
};
constexpr uint32_t kM26 = 0x3ffffff;

// d += a * b mod 2^130 - 5 (not carried; limbs of a and b below 2^27)
__device__ __forceinline__ void fe_mac(u64 d[5], const Fe& a, const Fe& b) {
  const u64 b0 = b.v[0], b1 = b.v[1], b2 = b.v[2], b3 = b.v[3], b4 = b.v[4];
  const u64 c1 = b1 * 5, c2 = b2 * 5, c3 = b3 * 5, c4 = b4 * 5;
  const u64 a0 = a.v[0], a1 = a.v[1], a2 = a.v[2], a3 = a.v[3], a4 = a.v[4];
  d[0] += a0 * b0 + a1 * c4 + a2 * c3 + a3 * c2 + a4 * c1;
  d[1] += a0 * b1 + a1 * b0 + a2 * c4 + a3 * c3 + a4 * c2;
  d[2] += a0 * b2 + a1 * b1 + a2 * b0 + a3 * c4 + a4 * c3;
  d[3] += a0 * b3 + a1 * b2 + a2 * b1 + a3 * b0 + a4 * c4;
  d[4] += a0 * b4 + a1 * b3 + a2 * b2 + a3 * b1 + a4 * b0;
}

// limbs below 2^26 (the second below 2^26 + 2^15) from sums below 2^62
__device__ __forceinline__ Fe fe_carry(const u64 d[5]) {
  u64 d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4], c;
  c = d0 >> 26, d0 &= kM26, d1 += c;
  c = d1 >> 26, d1 &= kM26, d2 += c;
  c = d2 >> 26, d2 &= kM26, d3 += c;
  c = d3 >> 26, d3 &= kM26, d4 += c;
  c = d4 >> 26, d4 &= kM26, d0 += c * 5;
  c = d0 >> 26, d0 &= kM26, d1 += c;
  Fe h;
  h.v[0] = (uint32_t)d0, h.v[1] = (uint32_t)d1, h.v[2] = (uint32_t)d2, h.v[3] = (uint32_t)d3,
  h.v[4] = (uint32_t)d4;
  return h;
}

__device__ __forceinline__ Fe fe_mul(const Fe& a, const Fe& b) {
  u64 d[5] = {0, 0, 0, 0, 0};
  fe_mac(d, a, b);
  return fe_carry(d);
}

// the 16 little-endian bytes w[0..3] plus hi * 2^128
__device__ __forceinline__ Fe fe_block(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t hi) {
  Fe m;
  m.v[0] = w0 & kM26;
  m.v[1] = ((w0 >> 26) | (w1 << 6)) & kM26;
  m.v[2] = ((w1 >> 20) | (w2 << 12)) & kM26;
  m.v[3] = ((w2 >> 14) | (w3 << 18)) & kM26;
  m.v[4] = (w3 >> 8) | (hi << 24);
  return m;
}

// r^e by square-and-multiply
__device__ __forceinline__ Fe fe_pow(Fe base, u64 e) {
  Fe x;
  x.v[0] = 1, x.v[1] = x.v[2] = x.v[3] = x.v[4] = 0;
  while (e) {
    if (e & 1) x = fe_mul(x, base);
    e >>= 1;
    if (e) base = fe_mul(base, base);
  }
  return x;
}

__device__ __forceinline__ Fe fe_load(const uint32_t* p) {
  Fe x;
  for (int k = 0; k < 5; ++k) x.v[k] = p[k];
  return x;
}

// the sum of d over the wave's lanes, in every lane's lane 0
__device__ __forceinline__ void wave_sum(u64 d[5]) {
  for (int off = 32; off; off >>= 1)
    for (int k = 0; k < 5; ++k) d[k] += __shfl_down(d[k], off, 64);
}

// ---- ChaCha20 ------------------------------------------------------------------------
#define DSX_QR(a, b, c, d)                       \
  a += b, d ^= a, d = __builtin_rotateleft32(d, 16); \
  c += d, b ^= c, b = __builtin_rotateleft32(b, 12); \
  a += b, d ^= a, d = __builtin_rotateleft32(d, 8);  \
  c += d, b ^= c, b = __builtin_rotateleft32(b, 7)

// 20 rounds over in[]; ADD: the block function (HChaCha20 leaves the sum out)
template <bool ADD>
__device__ __forceinline__ void chacha_rounds(const uint32_t in[16], uint32_t x[16]) {
  for (int k = 0; k < 16; ++k) x[k] = in[k];
#pragma unroll 1
  for (int r = 0; r < 10; ++r) {
    DSX_QR(x[0], x[4], x[8], x[12]);
    DSX_QR(x[1], x[5], x[9], x[13]);
    DSX_QR(x[2], x[6], x[10], x[14]);
    DSX_QR(x[3], x[7], x[11], x[15]);
    DSX_QR(x[0], x[5], x[10], x[15]);
    DSX_QR(x[1], x[6], x[11], x[12]);
    DSX_QR(x[2], x[7], x[8], x[13]);
    DSX_QR(x[3], x[4], x[9], x[14]);
  }
  if (ADD)
    for (int k = 0; k < 16; ++k) x[k] += in[k];
}

__device__ __forceinline__ void chacha_consts(uint32_t st[16]) {
  st[0] = 0x61707865, st[1] = 0x3320646e, st[2] = 0x79622d32, st[3] = 0x6b206574;
}

__device__ __forceinline__ uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// chunk i of the plaintext coordinates: [s, s + len) relative to start
__device__ __forceinline__ void chunk_span(const AeadArgs& a, u64 i, u64& s, u64& len) {
  const u64 e0 = i ? a.ends[i - 1] : a.start, e1 = a.ends[i];
  s = e0 - a.start;
  len = e1 - e0;
}

__device__ __forceinline__ u64 rec_off(const AeadArgs& a, u64 i, u64 s) {
  return a.offs ? a.offs[i] : s + 40 * i;
}

// ---- setup: one lane per record --------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void aead_setup_kernel(AeadArgs a, u64 i0) {
  const u64 i = i0 + (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  uint32_t* rc = a.rctx + i * kAeadCtxWords;
  uint32_t otk[8];
  if (MODE == kMac) {
    for (int k = 0; k < 8; ++k) otk[k] = le32(a.key + 4 * k);
  } else {
    u64 s, len;
    chunk_span(a, i, s, len);
    const u64 ro = rec_off(a, i, s);
    if (ro == kShort) return;  // (open: the finish marks it bad)
    uint8_t nonce[24];
    uint8_t* rn = a.rec + ro;
    if (MODE == kSeal)
      for (int k = 0; k < 24; ++k) rn[k] = nonce[k] = a.nonces[24 * i + k];
    else
      for (int k = 0; k < 24; ++k) nonce[k] = rn[k];
    uint32_t st[16], x[16];
    chacha_consts(st);
    for (int k = 0; k < 8; ++k) st[4 + k] = le32(a.key + 4 * k);
    for (int k = 0; k < 4; ++k) st[12 + k] = le32(nonce + 4 * k);
    chacha_rounds<false>(st, x);  // HChaCha20
    for (int k = 0; k < 4; ++k) st[4 + k] = x[k], st[8 + k] = x[12 + k];
    st[12] = 0, st[13] = 0, st[14] = le32(nonce + 16), st[15] = le32(nonce + 20);
    for (int k = 0; k < 8; ++k) rc[k] = st[4 + k];
    rc[8] = st[14], rc[9] = st[15];
    chacha_rounds<true>(st, x);  // block 0: the one-time key
    for (int k = 0; k < 8; ++k) otk[k] = x[k];
  }
  for (int k = 0; k < 4; ++k) rc[10 + k] = otk[4 + k];
  const Fe r1 = fe_block(otk[0] & 0x0fffffff, otk[1] & 0x0ffffffc, otk[2] & 0x0ffffffc,
                         otk[3] & 0x0ffffffc, 0);
  const Fe r2 = fe_mul(r1, r1), r3 = fe_mul(r2, r1), r4 = fe_mul(r2, r2);
  Fe big = r4;  // r^1024: a lane's next block lies 256 cipher blocks = 1024 MAC blocks on
  for (int k = 0; k < 8; ++k) big = fe_mul(big, big);
  for (int k = 0; k < 5; ++k) {
    rc[14 + k] = r1.v[k], rc[19 + k] = r2.v[k], rc[24 + k] = r3.v[k], rc[29 + k] = r4.v[k];
    rc[34 + k] = big.v[k];
  }
  rc[39] = 0;
}

// ---- main: one workgroup per tile ------------------------------------------------------
// Cipher blocks [b_lo, b_hi) of chunk i (len bytes, plaintext at pt, ciphertext at
// ct): lane t takes blocks b_lo + t, + 256, ...  The MAC runs over M = ceil(len /
// 16) + EXTRA blocks (EXTRA: the AEAD's length block), block j weighing r^(M - j).
// A piece of at most 64 blocks is one wave's (t = its lane, `active` in that wave
// only; the other waves write an empty slot), so that the pieces of small
// chunks run side by side on the workgroup's four waves.
template <int MODE>
__device__ __forceinline__ void aead_piece(const AeadArgs& a, u64 i, u64 k, uint8_t* pt, uint8_t* ct,
                                           u64 len, u64 b_lo, u64 b_hi, uint32_t t0, bool active) {
  constexpr u64 EXTRA = MODE == kMac ? 0 : 1;
  const uint32_t* rc = a.rctx + i * kAeadCtxWords;
  Fe rp[4];
  for (int e = 0; e < 4; ++e) rp[e] = fe_load(rc + 14 + 5 * e);
  const Fe big = fe_load(rc + 34);
  uint32_t st[16];
  if (MODE != kMac) {
    chacha_consts(st);
    for (int q = 0; q < 8; ++q) st[4 + q] = rc[q];
    st[13] = 0, st[14] = rc[8], st[15] = rc[9];
  }
  const u64 M = ((len + 15) >> 4) + EXTRA;
  u64 d[5] = {0, 0, 0, 0, 0};  // the lane's term of the piece's sum
  Fe acc;                      // full blocks so far, the last one weighing r^4 .. r
  bool have = false;
  u64 last = 0;
  for (u64 c = b_lo + t0; active && c < b_hi; c += kAeadThreads) {
    const u64 off = c << 6;
    const u64 rem = len - off;
    const bool full = rem >= 64;
    const uint8_t* src = (MODE == kSeal ? pt : ct) + off;
    uint8_t* dst = (MODE == kSeal ? ct : pt) + off;
    uint32_t w[16];
    if (full) {
      for (int q = 0; q < 4; ++q) {
        const a4u v = *(const DSX_AGLOBAL a4u_unaligned*)(src + 16 * q);
        w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
      }
    } else {
      const uint32_t nrem = (uint32_t)rem;
#pragma unroll
      for (int q = 0; q < 16; ++q) {  // (constant register indices: no scratch)
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint32_t at = 4 * q + b;
          if (at < nrem) v |= (uint32_t)src[at] << (8 * b);
          if (MODE == kMac && at == nrem) v |= 1u << (8 * b);  // raw Poly1305's pad byte
        }
        w[q] = v;
      }
    }
    if (MODE != kMac) {
      uint32_t x[16];
      st[12] = (uint32_t)(c + 1);
      chacha_rounds<true>(st, x);
      if (MODE == kOpen) {  // w stays the ciphertext, x becomes the plaintext
#pragma unroll
        for (int q = 0; q < 16; ++q) x[q] ^= w[q];
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) w[q] ^= x[q], x[q] = w[q];
      }
      if (full) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          a4u v;
          v.x = x[4 * q], v.y = x[4 * q + 1], v.z = x[4 * q + 2], v.w = x[4 * q + 3];
          *(DSX_AGLOBAL a4u_unaligned*)(dst + 16 * q) = v;
        }
      } else {
        const uint32_t nrem = (uint32_t)rem;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          uint32_t keep = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const uint32_t at = 4 * q + b;
            if (at < nrem) dst[at] = (uint8_t)(x[q] >> (8 * b)), keep |= 0xffu << (8 * b);
          }
          if (MODE == kSeal) w[q] &= keep;  // the MAC pads the ciphertext with zeros
        }
      }
    }
    if (full) {
      u64 t[5] = {0, 0, 0, 0, 0};
      if (have) fe_mac(t, acc, big);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        fe_mac(t, fe_block(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3], 1), rp[3 - q]);
      acc = fe_carry(t);
      have = true;
      last = c;
    } else {
      // the chunk's last, partial cipher block: Horner over its p MAC blocks,
      // then the length block's r; the term carries its final weight
      const uint32_t p = ((uint32_t)rem + 15) >> 4;
      Fe h;
      h.v[0] = h.v[1] = h.v[2] = h.v[3] = h.v[4] = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if ((uint32_t)q < p) {
          // raw Poly1305: a short last block has the pad byte instead of 2^128
          const uint32_t hi = (MODE == kMac && (uint32_t)q + 1 == p && (rem & 15)) ? 0 : 1;
          const Fe m = fe_block(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3], hi);
          for (int z = 0; z < 5; ++z) h.v[z] += m.v[z];
          h = fe_mul(h, rp[0]);
        }
      }
      if (EXTRA) h = fe_mul(h, rp[0]);
      for (int z = 0; z < 5; ++z) d[z] += h.v[z];
    }
  }
  if (have) {
    const Fe wgt = fe_pow(rp[0], M - 4 * last - 4);
    fe_mac(d, acc, wgt);
  }
  {
    const Fe h = fe_carry(d);  // (64 lanes of carried limbs stay far below 2^64)
    for (int z = 0; z < 5; ++z) d[z] = h.v[z];
  }
  wave_sum(d);
  if ((threadIdx.x & 63) == 0) {
    const Fe h = fe_carry(d);
    uint4* slot = reinterpret_cast<uint4*>(a.slots + ((i + k) * kAeadWaves + (threadIdx.x >> 6)) * kAeadSlotWords);
    slot[0] = make_uint4(h.v[0], h.v[1], h.v[2], h.v[3]);
    slot[1] = make_uint4(h.v[4], 0, 0, 0);
  }
}

template <int MODE>
__global__ __launch_bounds__(kAeadThreads) void aead_main_kernel(AeadArgs a, u64 tile0) {
  const u64 k = tile0 + blockIdx.x;
  const u64 lo = k * kTile;
  const u64 hi = std::min<u64>(lo + kTile, a.total);
  if (lo >= hi) return;
  // the first chunk that ends behind lo
  u64 l = 0, r = a.n;
  while (l < r) {
    const u64 m = (l + r) >> 1;
    if (a.ends[m] - a.start <= lo) l = m + 1;
    else r = m;
  }
  uint32_t small = 0;  // small pieces so far: they go round the waves
  for (u64 i = l; i < a.n; ++i) {
    u64 s, len;
    chunk_span(a, i, s, len);
    if (s >= hi) break;
    const u64 ro = rec_off(a, i, s);
    if (ro == kShort) continue;  // (no plaintext: len is 0)
    const u64 nblk = (len + 63) >> 6;
    const u64 b_lo = s >= lo ? 0 : (lo - s + 63) >> 6;
    const u64 b_hi = std::min<u64>(nblk, (hi - s + 63) >> 6);
    if (b_lo >= b_hi) continue;
    uint32_t t0 = threadIdx.x;
    bool active = true;
    if (b_hi - b_lo <= 64) {
      t0 &= 63;
      active = (threadIdx.x >> 6) == (small++ & (kAeadWaves - 1));
    }
    aead_piece<MODE>(a, i, k, a.pt + a.start + s, a.rec + ro + a.skip, len, b_lo, b_hi, t0, active);
  }
}

// ---- finish: one wave per record -------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void aead_finish_kernel(AeadArgs a, u64 i0) {
  const u64 i = i0 + (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (i >= a.n) return;
  u64 s, len;
  chunk_span(a, i, s, len);
  const u64 ro = rec_off(a, i, s);
  if (ro == kShort) {
    if (lane == 0) a.flag[i] = 1;
    return;
  }
  u64 d[5] = {0, 0, 0, 0, 0};
  if (len) {
    const u64 nblk = (len + 63) >> 6;
    const u64 k0 = s / kTile, k1 = (s + ((nblk - 1) << 6)) / kTile;
    const u64 cnt = (k1 - k0 + 1) * kAeadWaves;
    const uint32_t* base = a.slots + (i + k0) * kAeadWaves * kAeadSlotWords;
    u64 e = lane;
    for (; e + 192 < cnt; e += 256) {  // four slots in flight per lane
      uint4 v[4];
      uint32_t w[4];
      for (int q = 0; q < 4; ++q) {
        v[q] = *reinterpret_cast<const uint4*>(base + (e + 64 * q) * kAeadSlotWords);
        w[q] = base[(e + 64 * q) * kAeadSlotWords + 4];
      }
      for (int q = 0; q < 4; ++q)
        d[0] += v[q].x, d[1] += v[q].y, d[2] += v[q].z, d[3] += v[q].w, d[4] += w[q];
    }
    for (; e < cnt; e += 64) {
      const uint4 v = *reinterpret_cast<const uint4*>(base + e * kAeadSlotWords);
      d[0] += v.x, d[1] += v.y, d[2] += v.z, d[3] += v.w;
      d[4] += base[e * kAeadSlotWords + 4];
    }
  }
  wave_sum(d);
  if (lane != 0) return;
  const uint32_t* rc = a.rctx + i * kAeadCtxWords;
  if (MODE != kMac) {  // le64(0) || le64(len), times r
    const Fe lb = fe_block(0, 0, (uint32_t)len, (uint32_t)(len >> 32), 1);
    fe_mac(d, lb, fe_load(rc + 14));
  }
  Fe h = fe_carry(d);
  // the value mod 2^130 - 5: carry once more, then take h - p if it is not negative
  uint32_t c;
  c = h.v[1] >> 26, h.v[1] &= kM26, h.v[2] += c;
  c = h.v[2] >> 26, h.v[2] &= kM26, h.v[3] += c;
  c = h.v[3] >> 26, h.v[3] &= kM26, h.v[4] += c;
  c = h.v[4] >> 26, h.v[4] &= kM26, h.v[0] += c * 5;
  c = h.v[0] >> 26, h.v[0] &= kM26, h.v[1] += c;
  uint32_t g[5];
  g[0] = h.v[0] + 5, c = g[0] >> 26, g[0] &= kM26;
  g[1] = h.v[1] + c, c = g[1] >> 26, g[1] &= kM26;
  g[2] = h.v[2] + c, c = g[2] >> 26, g[2] &= kM26;
  g[3] = h.v[3] + c, c = g[3] >> 26, g[3] &= kM26;
  g[4] = h.v[4] + c - (1u << 26);
  const uint32_t take_g = (g[4] >> 31) - 1;  // all ones when h >= p
  for (int q = 0; q < 5; ++q) h.v[q] = (h.v[q] & ~take_g) | (g[q] & take_g);
  uint32_t t[4];
  t[0] = h.v[0] | (h.v[1] << 26);
  t[1] = (h.v[1] >> 6) | (h.v[2] << 20);
  t[2] = (h.v[2] >> 12) | (h.v[3] << 14);
  t[3] = (h.v[3] >> 18) | (h.v[4] << 8);
  u64 f = 0;
  for (int q = 0; q < 4; ++q) {  // + s mod 2^128
    f += (u64)t[q] + rc[10 + q];
    t[q] = (uint32_t)f;
    f >>= 32;
  }
  uint8_t* tag = MODE == kMac ? a.flag : a.rec + ro + a.skip + len;
  uint32_t diff = 0;
  for (int q = 0; q < 16; ++q) {
    const uint8_t b = (uint8_t)(t[q >> 2] >> (8 * (q & 3)));
    if (MODE == kOpen) diff |= (uint32_t)(tag[q] ^ b);  // every byte, no early exit
    else tag[q] = b;
  }
  if (MODE == kOpen) a.flag[i] = diff ? 1 : 0;
}

// ---- scrub: zero the plaintext of the records that failed --------------------------------
__global__ __launch_bounds__(kAeadThreads) void aead_scrub_kernel(AeadArgs a, u64 tile0) {
  const u64 k = tile0 + blockIdx.x;
  const u64 lo = k * kTile;
  const u64 hi = std::min<u64>(lo + kTile, a.total);
  if (lo >= hi) return;
  u64 l = 0, r = a.n;
  while (l < r) {
    const u64 m = (l + r) >> 1;
    if (a.ends[m] - a.start <= lo) l = m + 1;
    else r = m;
  }
  for (u64 i = l; i < a.n; ++i) {
    u64 s, len;
    chunk_span(a, i, s, len);
    if (s >= hi) break;
    if (!a.flag[i]) continue;
    const u64 b = std::max<u64>(s, lo), e = std::min<u64>(s + len, hi);
    uint8_t* p = a.pt + a.start;
    for (u64 x = b + threadIdx.x; x < e; x += kAeadThreads) p[x] = 0;
  }
}

}  // namespace dsx

using namespace dsx;

namespace {

// Clears what depends on the key.  Runs on every path out of a call that has
// uploaded it, a failed one included.
void aead_clear(dsx_ctx* c, uint64_t n, uint64_t slot_words) {
  AeadScratch& t = c->aead;
  hipStream_t st = c->stream;
  if (t.key.p) (void)hipMemsetAsync(t.key.p, 0, 32, st);
  if (t.rctx.p && n) (void)hipMemsetAsync(t.rctx.p, 0, n * kAeadCtxWords * 4, st);
  if (t.slots.p && slot_words) (void)hipMemsetAsync(t.slots.p, 0, slot_words * 4, st);
  (void)hipStreamSynchronize(st);
}

uint64_t slot_words_of(uint64_t n, uint64_t total) {
  return (n + total / kTile + 2) * kAeadWaves * kAeadSlotWords;
}

// setup, main and finish of one call on the ctx stream (not synchronised)
template <int MODE>
int aead_launches(dsx_ctx* c, const AeadArgs& a) {
  hipStream_t st = c->stream;
  for (uint64_t i0 = 0; i0 < a.n;) {
    const uint64_t nb = std::min<uint64_t>((a.n - i0 + 255) / 256, 1u << 22);
    hipLaunchKernelGGL(aead_setup_kernel<MODE>, dim3((uint32_t)nb), dim3(256), 0, st, a, (u64)i0);
    HIPCHK(c, hipGetLastError());
    i0 += nb * 256;
  }
  const uint64_t tiles = (a.total + kTile - 1) / kTile;
  for (uint64_t k0 = 0; k0 < tiles;) {
    const uint64_t nb = std::min<uint64_t>(tiles - k0, 1u << 30);
    hipLaunchKernelGGL(aead_main_kernel<MODE>, dim3((uint32_t)nb), dim3(kAeadThreads), 0, st, a, (u64)k0);
    HIPCHK(c, hipGetLastError());
    k0 += nb;
  }
  for (uint64_t i0 = 0; i0 < a.n;) {
    const uint64_t nb = std::min<uint64_t>((a.n - i0 + 3) / 4, 1u << 30);
    hipLaunchKernelGGL(aead_finish_kernel<MODE>, dim3((uint32_t)nb), dim3(256), 0, st, a, (u64)i0);
    HIPCHK(c, hipGetLastError());
    i0 += nb * 4;
  }
  return DSX_OK;
}

int aead_common_checks(dsx_ctx_t* c, int algo, const uint8_t* key, uint64_t n, uint32_t flags,
                       uint32_t allowed) {
  if (!c || !key) return DSX_E_INVAL;
  c->err.clear();
  if (algo != DSX_AEAD_XCHACHA20_POLY1305) return invalid(c, "unknown AEAD algorithm " + std::to_string(algo));
  if (flags & ~allowed) return invalid(c, "unknown flag bit");
  if (n > kCallMaxN) return invalid(c, "more than 0xFFFFFFF0 chunks");
  return DSX_OK;
}

}  // namespace

extern "C" int dsx_aead_seal(dsx_ctx_t* c, int algo, const uint8_t* key, const void* d_src,
                             uint64_t src_len, const uint64_t* ends, uint64_t start, uint64_t n,
                             const uint8_t* nonces, void* d_out, uint64_t out_cap,
                             uint64_t* out_ends, uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  int rc = aead_common_checks(c, algo, key, n, flags, DSX_ENDS_DEVICE);
  if (rc) return rc;
  if (n && (!ends || !d_out)) return DSX_E_INVAL;
  if (src_len && !d_src) return DSX_E_INVAL;
  if (!n) return DSX_OK;
  try {
    AeadScratch& t = c->aead;
    hipStream_t st = c->stream;
    std::vector<uint64_t> hends;
    const uint64_t* he = ends;
    if (flags & DSX_ENDS_DEVICE) {  // the list is checked on the host either way
      hends.resize(n);
      HIPCHK(c, hipSetDevice(c->device));
      HIPCHK(c, hipMemcpyAsync(hends.data(), ends, n * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
      he = hends.data();
    }
    uint64_t prev = start;
    for (uint64_t i = 0; i < n; ++i) {
      if (he[i] < prev)
        return invalid(c, "chunk " + std::to_string(i) + ": its end is below " +
                                 (i ? "the end before it" : "start"));
      if (he[i] > src_len) return invalid(c, "chunk " + std::to_string(i) + ": its end is beyond the buffer");
      if (he[i] - prev > kAeadMaxChunk)
        return invalid(c, "chunk " + std::to_string(i) + ": more than 2^38 - 64 bytes");
      prev = he[i];
    }
    const uint64_t total = he[n - 1] - start;
    const uint64_t need = total + kOverhead * n;
    if (need > out_cap) {
      c->err = "the records take " + std::to_string(need) + " bytes";
      return DSX_E_CAPACITY;
    }
    if (overlaps((const uint8_t*)d_src + start, total, d_out, need))
      return invalid(c, "the output overlaps the chunks");

    std::vector<uint8_t> drawn;
    if (!nonces) {  // crypto/rand.Read per chunk (encrypt.go:87)
      drawn.resize(n * kNonce);
      for (uint64_t got = 0; got < drawn.size();) {
        const ssize_t g = getrandom(drawn.data() + got, std::min<uint64_t>(drawn.size() - got, 1u << 20), 0);
        if (g < 0) {
          c->err = "getrandom failed";
          return DSX_E_IO;
        }
        got += (uint64_t)g;
      }
      // never the same nonce twice in a call: distinct leading words are enough
      std::unordered_set<uint64_t> seen;
      seen.reserve(n * 2);
      for (uint64_t i = 0; i < n; ++i) {
        uint64_t w;
        memcpy(&w, drawn.data() + kNonce * i, 8);
        while (!seen.insert(w).second) {
          if (getrandom(drawn.data() + kNonce * i, kNonce, 0) != (ssize_t)kNonce) {
            c->err = "getrandom failed";
            return DSX_E_IO;
          }
          memcpy(&w, drawn.data() + kNonce * i, 8);
        }
      }
      nonces = drawn.data();
    }

    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t sw = slot_words_of(n, total);
    HIPCHK(c, grow(c, t.key, 32));
    HIPCHK(c, grow(c, t.rctx, n * kAeadCtxWords));
    HIPCHK(c, grow(c, t.slots, sw));
    HIPCHK(c, grow(c, t.nonces, n * kNonce));
    AeadArgs a{};
    if (flags & DSX_ENDS_DEVICE) {
      a.ends = (const u64*)ends;
    } else {
      HIPCHK(c, grow(c, t.ends, n));
      HIPCHK(c, hipMemcpyAsync(t.ends.p, ends, n * 8, hipMemcpyHostToDevice, st));
      a.ends = t.ends.p;
    }
    HIPCHK(c, hipMemcpyAsync(t.nonces.p, nonces, n * kNonce, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(t.key.p, key, 32, hipMemcpyHostToDevice, st));
    a.start = start, a.n = n, a.total = total, a.offs = nullptr;
    a.pt = (uint8_t*)const_cast<void*>(d_src), a.rec = (uint8_t*)d_out, a.skip = kNonce;
    a.rctx = t.rctx.p, a.slots = t.slots.p, a.flag = nullptr, a.key = t.key.p, a.nonces = t.nonces.p;
    rc = aead_launches<kSeal>(c, a);
    aead_clear(c, n, sw);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (out_ends)
      for (uint64_t i = 0; i < n; ++i) out_ends[i] = (he[i] - start) + kOverhead * (i + 1);
    return DSX_OK;
  } catch (const std::bad_alloc&) {
    return DSX_E_NOMEM;
  }
}

extern "C" int dsx_aead_open(dsx_ctx_t* c, int algo, const uint8_t* key, const void* d_in,
                             uint64_t in_len, const uint64_t* rec_ends, uint64_t start, uint64_t n,
                             void* d_out, uint64_t out_cap, uint64_t* out_ends, uint32_t* bad,
                             uint64_t cap, uint64_t* n_bad, uint32_t flags) {
  DSX_FLUSH_BEHIND(c);
  int rc = aead_common_checks(c, algo, key, n, flags, 0);
  if (rc) return rc;
  if (!n_bad || (cap && !bad)) return DSX_E_INVAL;
  if (n && !rec_ends) return DSX_E_INVAL;
  if (in_len && !d_in) return DSX_E_INVAL;
  *n_bad = 0;
  if (!n) return DSX_OK;
  try {
    std::vector<uint64_t> pe(n), offs(n);
    uint64_t prev = start, total = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (rec_ends[i] < prev)
        return invalid(c, "record " + std::to_string(i) + ": its end is below " +
                                 (i ? "the end before it" : "start"));
      if (rec_ends[i] > in_len) return invalid(c, "record " + std::to_string(i) + ": its end is beyond the buffer");
      const uint64_t size = rec_ends[i] - prev;
      const uint64_t len = size >= kOverhead ? size - kOverhead : 0;
      if (len > kAeadMaxChunk)
        return invalid(c, "record " + std::to_string(i) + ": more than 2^38 - 64 bytes of ciphertext");
      offs[i] = size >= kOverhead ? prev : kShort;
      total += len;
      pe[i] = total;
      prev = rec_ends[i];
    }
    if (total > out_cap) {
      c->err = "the plaintext takes " + std::to_string(total) + " bytes";
      return DSX_E_CAPACITY;
    }
    if (total && !d_out) return DSX_E_INVAL;
    if (overlaps((const uint8_t*)d_in + start, rec_ends[n - 1] - start, d_out, total))
      return invalid(c, "the output overlaps the records");

    AeadScratch& t = c->aead;
    hipStream_t st = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t sw = slot_words_of(n, total);
    HIPCHK(c, grow(c, t.key, 32));
    HIPCHK(c, grow(c, t.rctx, n * kAeadCtxWords));
    HIPCHK(c, grow(c, t.slots, sw));
    HIPCHK(c, grow(c, t.ends, n));
    HIPCHK(c, grow(c, t.offs, n));
    HIPCHK(c, grow(c, t.flag, std::max<uint64_t>(n, 16)));
    HIPCHK(c, hipMemcpyAsync(t.ends.p, pe.data(), n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(t.offs.p, offs.data(), n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(t.key.p, key, 32, hipMemcpyHostToDevice, st));
    AeadArgs a{};
    a.ends = t.ends.p, a.start = 0, a.n = n, a.total = total, a.offs = t.offs.p;
    a.pt = (uint8_t*)d_out, a.rec = (uint8_t*)const_cast<void*>(d_in), a.skip = kNonce;
    a.rctx = t.rctx.p, a.slots = t.slots.p, a.flag = t.flag.p, a.key = t.key.p, a.nonces = nullptr;
    rc = aead_launches<kOpen>(c, a);
    aead_clear(c, n, sw);
    if (rc) return rc;
    std::vector<uint8_t> hflag(n);
    HIPCHK(c, hipMemcpyAsync(hflag.data(), t.flag.p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    uint64_t nb = 0;
    for (uint64_t i = 0; i < n; ++i)
      if (hflag[i]) {
        if (nb < cap) bad[nb] = (uint32_t)i;
        ++nb;
      }
    if (nb && total) {  // Open releases no plaintext of a record that failed
      const uint64_t tiles = (total + kTile - 1) / kTile;
      for (uint64_t k0 = 0; k0 < tiles;) {
        const uint64_t g = std::min<uint64_t>(tiles - k0, 1u << 30);
        hipLaunchKernelGGL(aead_scrub_kernel, dim3((uint32_t)g), dim3(kAeadThreads), 0, st, a, (u64)k0);
        HIPCHK(c, hipGetLastError());
        k0 += g;
      }
      HIPCHK(c, hipStreamSynchronize(st));
    }
    *n_bad = nb;
    if (out_ends) memcpy(out_ends, pe.data(), n * 8);
    return DSX_OK;
  } catch (const std::bad_alloc&) {
    return DSX_E_NOMEM;
  }
}

extern "C" int dsx_selftest_poly1305(dsx_ctx_t* c, const uint8_t* otk, const void* d_msg, uint64_t len,
                                     uint8_t* tag) {
  DSX_FLUSH_BEHIND(c);
  if (!c || !otk || !tag || (len && !d_msg)) return DSX_E_INVAL;
  c->err.clear();
  AeadScratch& t = c->aead;
  hipStream_t st = c->stream;
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t sw = slot_words_of(1, len);
  HIPCHK(c, grow(c, t.key, 32));
  HIPCHK(c, grow(c, t.rctx, kAeadCtxWords));
  HIPCHK(c, grow(c, t.slots, sw));
  HIPCHK(c, grow(c, t.ends, 1));
  HIPCHK(c, grow(c, t.offs, 1));
  HIPCHK(c, grow(c, t.flag, 16));
  const uint64_t zero = 0;
  HIPCHK(c, hipMemcpyAsync(t.ends.p, &len, 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(t.offs.p, &zero, 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(t.key.p, otk, 32, hipMemcpyHostToDevice, st));
  AeadArgs a{};
  a.ends = t.ends.p, a.start = 0, a.n = 1, a.total = len, a.offs = t.offs.p;
  a.pt = nullptr, a.rec = (uint8_t*)const_cast<void*>(d_msg), a.skip = 0;
  a.rctx = t.rctx.p, a.slots = t.slots.p, a.flag = t.flag.p, a.key = t.key.p, a.nonces = nullptr;
  const int rc = aead_launches<kMac>(c, a);
  if (!rc) (void)hipMemcpyAsync(tag, t.flag.p, 16, hipMemcpyDeviceToHost, st);
  aead_clear(c, 1, sw);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  return DSX_OK;
}
