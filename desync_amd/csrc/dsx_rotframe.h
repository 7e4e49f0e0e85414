// dsx_rotframe.h -- the rotating frame of scanl_kernel<..., ROTF> (DESIGN.md
// 4.1, "Rotating frame").  Host- and device-compilable: the kernel and the CPU
// model of tests/test_rotframe_model.py take the slot, rotation and register
// packing arithmetic from here.
//
// MODE 2 rolls x = ~h with
//     x_i = rotl1(x_{i-1}) ^ T[b_i] ^ rotl16(T[b_{i-48}]).
// The rotating frame keeps g_i = rotl^{s_i}(x_i) with a per-lane rotation that
// falls by one each byte, s_i = (lane - i) mod 32.  Then
//     g_i = g_{i-1} ^ U_i ^ U_{i-48},      U_i = rotl^{s_i}(T[b_i]),
// because s_{i-1} = s_i + 1 and s_{i-48} = s_i + 48 = s_i + 16 (mod 32): the
// outgoing term IS the value looked up 48 bytes earlier, so the table holds
// no rotl16 copy and no rotate sits in the recurrence.  x_i = rotr^{s_i}(g_i)
// is one v_alignbit_b32 in front of the unchanged boundary test.
//
// Stream positions i of a lane segment: byte p of trip t is i = 384*t + p,
// byte q of the 48-byte warm-up i = q - 48, byte p' of the handoff extension
// i = 384*M + p'.  384 = 12*32 = 6*64, so the phase i mod 32 and the ring
// register i mod 64 are static per code position.
#ifndef DSX_ROTFRAME_H_
#define DSX_ROTFRAME_H_
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSX_RF_HD __host__ __device__
#else
#define DSX_RF_HD
#endif

namespace dsx {
namespace rotframe {

constexpr int kWindow = 48;  // Buzhash window
constexpr int kPhases = 32;  // per-lane phase registers, one per i mod 32
constexpr int kSlots = 64;   // table slots per byte value (4 B each, one per LDS bank)
constexpr int kRing = 64;    // lookups kept: register i mod 64
constexpr int kTableBytes = 256 * kSlots * 4;

DSX_RF_HD constexpr uint32_t rotl32(uint32_t x, uint32_t s) {
  return (s & 31u) ? (x << (s & 31u)) | (x >> (32u - (s & 31u))) : x;
}
DSX_RF_HD constexpr uint32_t rotr32(uint32_t x, uint32_t s) { return rotl32(x, 32u - (s & 31u)); }

// i mod n for i >= -64 (the warm-up positions are -48 .. -1)
DSX_RF_HD constexpr int phase_of(int i) { return (i + 2 * kPhases) % kPhases; }
// The ring: the lookup of i + 64 rewrites the register of i, which is last
// read as the outgoing term of i + 48.  With the lookups one subgroup of 8
// bytes ahead, those of positions up to 8j + 15 are issued while subgroup j
// still reads the registers of 8j + 16 .. 8j + 23 as outgoing terms: no
// overlap.  (Two subgroups ahead would need more registers: 96 divides 384.)
DSX_RF_HD constexpr int ring_in(int i) { return (i + kRing) % kRing; }  // lookup of i lands here
DSX_RF_HD constexpr int ring_out(int i) { return (i - kWindow + 2 * kRing) % kRing; }  // == ring_in(i - 48)

// Table slot that `lane` reads in phase `phase`.  For a fixed phase this maps
// the 64 lanes onto the 64 slots one to one (the low five bits are a shift of
// the lane's, bit 5 is kept), and slot k of a byte value is LDS bank k: a
// ds_read_b32 of the whole wave is conflict-free whatever the bytes are.
DSX_RF_HD constexpr uint32_t slot_of(uint32_t lane, uint32_t phase) {
  return ((lane - phase) & 31u) | (lane & 32u);
}
// Left rotation of the table values in a slot; the upper 32 slots repeat the
// lower 32.  slot_rot(slot_of(lane, i)) is s_i.
DSX_RF_HD constexpr uint32_t slot_rot(uint32_t slot) { return slot & 31u; }
// LDS byte offset of slot `slot` of byte value v, and the value kept there
DSX_RF_HD constexpr uint32_t table_offset(uint32_t v, uint32_t slot) { return v * 256u + slot * 4u; }
DSX_RF_HD constexpr uint32_t table_value(uint32_t tv, uint32_t slot) { return rotl32(tv, slot_rot(slot)); }

// A phase register: byte 0 = s (v_alignbit_b32 reads bits [4:0] of its shift
// operand), byte 1 = slot * 4 (v_perm_b32 moves it to byte 0 of the address).
DSX_RF_HD constexpr uint32_t phase_reg(uint32_t lane, uint32_t phase) {
  return slot_rot(slot_of(lane, phase)) | ((slot_of(lane, phase) * 4u) << 8);
}
DSX_RF_HD constexpr uint32_t phase_reg_rot(uint32_t pr) { return pr & 31u; }
// table_offset(byte k of w, the phase's slot): what v_perm_b32(w, pr,
// lookup_sel(k)) computes
DSX_RF_HD constexpr uint32_t lookup_sel(int k) { return 0x0C0C0001u | ((4u + (uint32_t)k) << 8); }
DSX_RF_HD constexpr uint32_t lookup_offset(uint32_t w, uint32_t pr, int k) {
  return (((w >> (8 * k)) & 0xFFu) << 8) | ((pr >> 8) & 0xFFu);
}

// x_i from g_i (plain form of the kernel's v_alignbit_b32(g, g, pr))
DSX_RF_HD constexpr uint32_t unrotate(uint32_t g, uint32_t pr) { return rotr32(g, phase_reg_rot(pr)); }

}  // namespace rotframe
}  // namespace dsx
#endif  // DSX_ROTFRAME_H_
