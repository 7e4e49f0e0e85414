// dsx_scan_geom.h -- the scan geometry of one piece as a pure function: how a
// piece is cut into lane segments and regions, the region-list capacity, the
// line-grid origin and the launch grid (DESIGN.md "Scan kernel").  Integer
// arithmetic only, no HIP: enqueue_piece (dsx_engine.cpp) fills ScanArgs and
// PieceCands from it, and tests/test_scan_geom_model.py runs it on the CPU.
#ifndef DSX_SCAN_GEOM_H_
#define DSX_SCAN_GEOM_H_
#include <stdint.h>

#include <algorithm>

#include "dsx_common.h"

namespace dsx_host {

constexpr uint32_t kDenseS = 48 * 9;  // dense path lane bytes (= slot cap)

// scan configs (DSX_SCAN_CFG): {waves per workgroup, rounds per DMA batch}
constexpr int kCfgWaves[6] = {8, 12, 16, 12, 8, 16};
constexpr int kCfgBR[6] = {2, 1, 1, 2, 2, 2};

struct ScanGeomIn {
  uint64_t len = 0;   // piece [P, P + len) ...
  uint64_t P = 0;
  uint64_t halo = 0;  // ... with `halo` readable bytes before it
  uint32_t delta = 0;          // the piece pointer's offset in its 128-B line
  uint32_t discriminator = 0;  // dsx_params_t.discriminator
  bool dense = false;          // CallCfg.dense
  bool behind = false;         // CallCfg.behind
  // the context's settings (dsx_ctx, dsx_engine.h)
  bool scan_line = true;
  int scan_cfg = 0;
  int scanl_waves = 8;
  int ncu = 256;
  int stitch_cus = 0;
  bool split = false;  // split streams: the scan leaves stitch_cus CUs free
  int regions_per_slot = 1;
  uint32_t lane_target = 8448;
  uint32_t lane_bytes_override = 0;
  int tail_split = 4;
  int tail_mult = 1;
};

struct ScanGeom {
  bool line = false;     // scanl_kernel (else scan_kernel, 96-B rows)
  int W = 0;             // waves per workgroup
  uint32_t S = 0;        // lane segment bytes
  uint32_t LS = 0;       // candidate slots per lane
  uint32_t batches = 0;  // DMA batches (line: trips of 384 B) per lane segment
  uint64_t region_bytes = 0;  // 64 * S
  uint64_t nregions = 0;
  // two region sizes: regions [nbig, nregions) have lane segments of S2 bytes
  // (batches2 trips, region_bytes2 bytes); S2 == 0: one size, nbig == nregions
  uint64_t nbig = 0;
  uint64_t S2 = 0;
  uint32_t batches2 = 0;
  uint64_t region_bytes2 = 0;
  uint32_t rcap = 0;     // region-list capacity
  uint64_t nlanes = 0;   // nregions * 64
  uint32_t delta = 0;    // line scan: ScanArgs.delta and .shift0 (else 0)
  uint32_t shift0 = 0;
  uint64_t grid_P = 0;   // region r covers (grid_P + base(r), grid_P + base(r) + bytes(r)]
  uint32_t grid = 0;     // workgroups of W waves
};

inline ScanGeom scan_geom(const ScanGeomIn& in) {
  using namespace dsx;
  const uint64_t len = in.len;
  ScanGeom g;
  // ---- scan geometry: balance regions over the persistent grid ----
  // lane segment S = 48*(4k-1): the warm-up round plus S/48 rounds fill k
  // whole 4-round DMA batches
  // line-aligned scan (scanl_kernel) unless disabled, on the dense path, or
  // when the grid origin P - delta would precede position 0
  const uint32_t delta = in.delta;
  const bool line = in.scan_line && !in.dense && in.P >= delta;
  const int W = line ? in.scanl_waves : kCfgWaves[in.scan_cfg];
  const int cfgBR = kCfgBR[in.scan_cfg];
  const int ncu_scan = in.ncu - (in.split ? in.stitch_cus : 0);  // CUs of the scan's mask
  const uint64_t slots_total = (uint64_t)ncu_scan * W;            // wave slots
  const uint64_t span = line ? len + delta : len;                 // grid bytes
  uint32_t S, LS;
  uint32_t batches;
  if (in.dense) {
    S = kDenseS;
    LS = S;
  } else if (line) {
    // S = 384*m: about regions_per_slot regions per wave slot
    const uint64_t lanes_min = slots_total * 64 * (uint64_t)in.regions_per_slot;
    const uint64_t per_lane = (span + lanes_min - 1) / lanes_min;
    const uint64_t rounds_needed = (per_lane + kLineLaneMax - 1) / kLineLaneMax;
    const uint64_t s = (span + rounds_needed * lanes_min - 1) / (rounds_needed * lanes_min);
    uint64_t m = (s + 3 * kLine - 1) / (3 * kLine);
    // lane segments longer than the target lose HBM efficiency (lane stride
    // 33 KB: 4.85 TB/s staging vs 6.24 TB/s at 8448 B, tools/ubench_staging.hip);
    // bigger pieces take more regions per wave slot from the work queue
    // (up to two trips past the target when that keeps every region in the
    // first pass: a second pass for a few regions costs a whole region time)
    const uint64_t mcap = in.lane_target / (3 * kLine);
    if (m > mcap + mcap / 4 || rounds_needed > 1) m = std::min<uint64_t>(m, mcap);
    m = std::max<uint64_t>(1, std::min<uint64_t>(m, kLineLaneMax / (3 * kLine)));
    S = (uint32_t)(3 * kLine * m);
    if (in.lane_bytes_override && in.lane_bytes_override % (3 * kLine) == 0 &&
        in.lane_bytes_override <= kLineLaneMax)
      S = in.lane_bytes_override;
    LS = kLaneSlots;
  } else {
    // about regions_per_slot regions per wave slot (dynamic queue balances
    // them), more if a lane segment would exceed kMaxLaneBytes
    const uint64_t lanes_min = slots_total * 64 * (uint64_t)in.regions_per_slot;
    const uint64_t per_lane = (len + lanes_min - 1) / lanes_min;
    const uint64_t rounds_needed = (per_lane + kMaxLaneBytes - 1) / kMaxLaneBytes;
    uint64_t s = (len + rounds_needed * lanes_min - 1) / (rounds_needed * lanes_min);
    const uint64_t BR = (uint64_t)cfgBR;
    uint64_t kb = (s / kRound + 1 + BR - 1) / BR;  // batches
    if (kb < 4) kb = 4;
    while (kRound * (BR * kb - 1) > kMaxLaneBytes) --kb;
    s = (uint64_t)kRound * (BR * kb - 1);
    if (in.lane_bytes_override && (in.lane_bytes_override / kRound + 1) % BR == 0)
      s = in.lane_bytes_override;
    S = (uint32_t)s;
    LS = kLaneSlots;
  }
  batches = line ? S / (3 * kLine) : (S / kRound + 1) / (uint32_t)cfgBR;
  const uint64_t region_bytes = 64ull * S;
  uint64_t nregions = len == 0 ? 0 : (span + region_bytes - 1) / region_bytes;
  // Two region sizes (DSX_TAIL_SPLIT = k > 1, default 4; line scan, pieces of
  // at least three big regions per wave slot): the last ~one big region's
  // worth of bytes per wave slot is cut into regions with k times shorter lane
  // segments, so the waves that drain the work queue last hold small regions
  // (DSX_TAIL_MULT = j: j big regions' worth per wave slot).  On the 8 GiB
  // pieces the waves end together (wave_busy 0.947 -> 0.98) and the scan is
  // 1 % faster; k = 2, 6, 8 and j = 2 less (profiles/r04d, r04e, r04g, r04aa).
  // (k = 3 was the default while every lane read a warm-up line: k = 4 read
  // 1.021 x the input against 1.018; since the warm-up handoff only lane 0 of
  // a region does, and k = 4 is 0.4-0.5 % ahead, profiles/r04ab.)
  uint64_t nbig = nregions, S2 = 0;
  if (line && !in.dense && !in.behind && in.tail_split > 1 && len > 0) {
    const uint64_t m = S / (3 * kLine), m2 = std::max<uint64_t>(1, m / (uint64_t)in.tail_split);
    const uint64_t tail = slots_total * region_bytes * (uint64_t)in.tail_mult;
    if (m2 < m && span >= 3 * tail) {
      const uint64_t rb2 = 64ull * 3 * kLine * m2;
      nbig = (span - tail) / region_bytes;
      nregions = nbig + (span - nbig * region_bytes + rb2 - 1) / rb2;
      S2 = 3 * kLine * m2;
    }
  }
  const uint64_t nlanes = nregions * 64;
  uint32_t rcap;
  if (in.dense) {
    rcap = 64u * S;
  } else {
    const double expct = (double)region_bytes / (double)in.discriminator;
    rcap = (uint32_t)std::min<double>(64.0 * S, 4.0 * expct + 64.0);
    rcap = (rcap + 63u) & ~63u;
  }
  if (line) {
    // region 0's descriptor: the warm-up line unless it would start before
    // the readable bytes (then the 16-B step at or below base - min(halo, 48))
    const uint64_t hmin = std::min<uint64_t>(in.halo, kRound);
    g.delta = delta;
    g.shift0 = in.halo >= (uint64_t)delta + kLine
                   ? 0u
                   : (uint32_t)(16 * (((uint64_t)kLine + delta - hmin) / 16));
  }
  const uint64_t need_wg = std::max<uint64_t>(1, (nregions + W - 1) / W);
  // (stitch behind: every CU, so the wave slots beyond the regions -- spread
  // over the grid by the wave-major order -- run the tasks from the start)
  g.grid = in.behind ? (uint32_t)ncu_scan
                     : (uint32_t)std::min<uint64_t>(need_wg, (uint64_t)ncu_scan);
  g.line = line;
  g.W = W;
  g.S = S;
  g.LS = LS;
  g.batches = batches;
  g.region_bytes = region_bytes;
  g.nregions = nregions;
  g.nbig = nbig;
  g.S2 = S2;
  g.batches2 = (uint32_t)(S2 / (3 * kLine));
  g.region_bytes2 = S2 ? 64ull * S2 : 0;
  g.rcap = rcap;
  g.nlanes = nlanes;
  g.grid_P = line ? in.P - delta : in.P;
  return g;
}

}  // namespace dsx_host

#endif  // DSX_SCAN_GEOM_H_
