// dsx_aead.h -- the XChaCha20-Poly1305 store converter (dsx_aead.hip): what a
// context holds for it.  Included by dsx_engine.h behind dsx_store.h.
#pragma once

#include <stdint.h>

struct dsx_ctx;

// Plaintext bytes one workgroup of the main pass owns.
constexpr uint64_t kAeadTile = 262144;
// Words of one record's context: subkey[8], nonce words[2], s[4], then r, r^2,
// r^3, r^4 and r^1024 as five 26-bit limbs each, one word of padding.
constexpr int kAeadCtxWords = 40;
// Words of one partial slot (five limbs, padded to two 16-byte stores), and the
// slots one (chunk, tile) pair has: one per wave of the workgroup.
constexpr int kAeadSlotWords = 8;
constexpr int kAeadWaves = 4;

// The scratch of a seal / open / selftest call.  Grows once, reused; key, rctx
// and slots are cleared before each call returns.
struct AeadScratch {
  DevBuf<uint8_t> key;              // the 32-byte key (selftest: the one-time key)
  DevBuf<uint32_t> rctx;            // n * kAeadCtxWords
  DevBuf<uint32_t> slots;           // (n + tiles + 1) * kAeadWaves * kAeadSlotWords
  DevBuf<unsigned long long> ends;  // staged host ends (open: the plaintext ends)
  DevBuf<unsigned long long> offs;  // open: the records' offsets (UINT64_MAX: too short)
  DevBuf<uint8_t> nonces;           // seal: n * 24
  DevBuf<uint8_t> flag;             // open: bad[i]; selftest: the tag
};
