// The scan geometry (desync_amd/csrc/dsx_scan_geom.h) on the CPU, built and
// run by tests/test_scan_geom_model.py:
//   g++ -std=c++17 -O1 -g -Wall -Werror -Iinclude -Idesync_amd/csrc
//       tests/scan_geom_model.cpp
// The test uses no sanitizer.  A sanitizer run is a build by hand of this same
// stand-alone program, with
//   -fsanitize=address,undefined -fno-sanitize-recover=all
// added to that line.
//
// a. kRows pins scan_geom()'s whole output for the smallest shapes on each
//    side of every branch.  The expected values were recorded from the
//    arithmetic enqueue_piece carried inline before the geometry became this
//    header (a copy of those lines printed the rows), not from the header.
// b. A seeded sweep of line-scan pieces checks what the kernels and
//    pc_region_base / pc_region_of (dsx_stitch.h) rely on.
// c. At the defaults S is 768 exactly when len + delta > 384 * lanes (spans up
//    to 768 * lanes), else 384: the rule tests/test_gpu_seam_record.py
//    restates in _geometry.
#include <stdint.h>
#include <stdio.h>

#include "dsx_scan_geom.h"

using dsx_host::scan_geom;
using dsx_host::ScanGeom;
using dsx_host::ScanGeomIn;

struct Row {
  const char* name;
  // len, P, halo, delta, discriminator, dense, behind, scan_line, scan_cfg,
  // scanl_waves, ncu, stitch_cus, split, regions_per_slot, lane_target,
  // lane_bytes_override, tail_split, tail_mult
  ScanGeomIn in;
  // line, W, S, LS, batches, region_bytes, nregions, nbig, S2, batches2,
  // region_bytes2, rcap, nlanes, delta, shift0, grid_P, grid
  ScanGeom out;
};

// Unless the name says otherwise: P = halo = 1 MiB, 256 CUs, 8 waves,
// tail_split 4, tail_mult 1, lane_target 8448, one region per slot,
// discriminator 49535.  lanes = 256 * 8 * 64, tail = 2048 * 540672.
static const Row kRows[] = {
    {"len 1",
     {1ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 1ull, 1ull, 0ull, 0u, 0ull, 128u, 64ull, 0u, 0u, 1048576ull, 1u}},
    {"len 47",
     {47ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 1ull, 1ull, 0ull, 0u, 0ull, 128u, 64ull, 0u, 0u, 1048576ull, 1u}},
    {"len 48",
     {48ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 1ull, 1ull, 0ull, 0u, 0ull, 128u, 64ull, 0u, 0u, 1048576ull, 1u}},
    {"len 49",
     {49ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 1ull, 1ull, 0ull, 0u, 0ull, 128u, 64ull, 0u, 0u, 1048576ull, 1u}},
    {"len 383",
     {383ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 1ull, 1ull, 0ull, 0u, 0ull, 128u, 64ull, 0u, 0u, 1048576ull, 1u}},
    {"one trip: 384*lanes",
     {50331648ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 2048ull, 2048ull, 0ull, 0u, 0ull, 128u, 131072ull, 0u, 0u, 1048576ull, 256u}},
    {"two trips: 384*lanes + 1",
     {50331649ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 1025ull, 1025ull, 0ull, 0u, 0ull, 128u, 65600ull, 0u, 0u, 1048576ull, 129u}},
    {"384*lanes, delta 73",
     {50331648ull, 1048576ull, 1048576ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 1025ull, 1025ull, 0ull, 0u, 0ull, 128u, 65600ull, 73u, 0u, 1048503ull, 129u}},
    {"384*lanes + 1, delta 73",
     {50331649ull, 1048576ull, 1048576ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 1025ull, 1025ull, 0ull, 0u, 0ull, 128u, 65600ull, 73u, 0u, 1048503ull, 129u}},
    {"span 384*lanes, delta 73",
     {50331575ull, 1048576ull, 1048576ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 2048ull, 2048ull, 0ull, 0u, 0ull, 128u, 131072ull, 73u, 0u, 1048503ull, 256u}},
    {"span 384*lanes + 1, delta 73",
     {50331576ull, 1048576ull, 1048576ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 1025ull, 1025ull, 0ull, 0u, 0ull, 128u, 65600ull, 73u, 0u, 1048503ull, 129u}},
    {"delta 0",
     {1048581ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 0u, 0u, 1048576ull, 6u}},
    {"delta 73",
     {1048581ull, 1048576ull, 1048576ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 73u, 0u, 1048503ull, 6u}},
    {"delta 127",
     {1048581ull, 1048576ull, 1048576ull, 127u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 127u, 0u, 1048449ull, 6u}},
    {"P 0, delta 73: row kernel",
     {1048581ull, 0ull, 0ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {false, 8, 336u, 32u, 4u, 21504ull, 49ull, 49ull, 0ull, 0u, 0ull, 128u, 3136ull, 0u, 0u, 0ull, 7u}},
    {"P 0, delta 0, halo 0",
     {1048581ull, 0ull, 0ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 0u, 128u, 0ull, 6u}},
    {"halo 0",
     {1048581ull, 1048576ull, 0ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 73u, 192u, 1048503ull, 6u}},
    {"halo 47",
     {1048581ull, 1048576ull, 47ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 73u, 144u, 1048503ull, 6u}},
    {"halo 48",
     {1048581ull, 1048576ull, 48ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 73u, 144u, 1048503ull, 6u}},
    {"halo delta + 127",
     {1048581ull, 1048576ull, 200ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 73u, 144u, 1048503ull, 6u}},
    {"halo delta + 128",
     {1048581ull, 1048576ull, 201ull, 73u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 73u, 0u, 1048503ull, 6u}},
    {"1 GiB aligned",
     {1073741824ull, 0ull, 0ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 1986ull, 1986ull, 0ull, 0u, 0ull, 128u, 127104ull, 0u, 128u, 0ull, 249u}},
    {"8 GiB aligned",
     {8589934592ull, 0ull, 0ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 22853ull, 13839ull, 1920ull, 5u, 122880ull, 128u, 1462592ull, 0u, 128u, 0ull, 256u}},
    {"span 3*tail - 1",
     {3321888767ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 6144ull, 6144ull, 0ull, 0u, 0ull, 128u, 393216ull, 0u, 0u, 1048576ull, 256u}},
    {"span 3*tail",
     {3321888768ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 13108ull, 4096ull, 1920ull, 5u, 122880ull, 128u, 838912ull, 0u, 0u, 1048576ull, 256u}},
    {"8 GiB, tail_split 0",
     {8589934592ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 0, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 15888ull, 15888ull, 0ull, 0u, 0ull, 128u, 1016832ull, 0u, 0u, 1048576ull, 256u}},
    {"8 GiB, tail_split 1",
     {8589934592ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 1, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 15888ull, 15888ull, 0ull, 0u, 0ull, 128u, 1016832ull, 0u, 0u, 1048576ull, 256u}},
    {"8 GiB, tail_split 3",
     {8589934592ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 3, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 20278ull, 13839ull, 2688ull, 7u, 172032ull, 128u, 1297792ull, 0u, 0u, 1048576ull, 256u}},
    {"8 GiB, tail_split 4",
     {8589934592ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 22853ull, 13839ull, 1920ull, 5u, 122880ull, 128u, 1462592ull, 0u, 0u, 1048576ull, 256u}},
    {"8 GiB, tail_mult 2",
     {8589934592ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 2},
     {true, 8, 8448u, 32u, 22u, 540672ull, 29816ull, 11791ull, 1920ull, 5u, 122880ull, 128u, 1908224ull, 0u, 0u, 1048576ull, 256u}},
    {"8 GiB, behind",
     {8589934592ull, 1048576ull, 1048576ull, 0u, 49535u, false, true, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 15888ull, 15888ull, 0ull, 0u, 0ull, 128u, 1016832ull, 0u, 0u, 1048576ull, 256u}},
    {"64 MiB, behind",
     {67108864ull, 1048576ull, 1048576ull, 0u, 49535u, false, true, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 1366ull, 1366ull, 0ull, 0u, 0ull, 128u, 87424ull, 0u, 0u, 1048576ull, 256u}},
    {"64 MiB",
     {67108864ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 1366ull, 1366ull, 0ull, 0u, 0ull, 128u, 87424ull, 0u, 0u, 1048576ull, 171u}},
    {"64 MiB, lane_target 384",
     {67108864ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 384u, 0u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 2731ull, 2731ull, 0ull, 0u, 0ull, 128u, 174784ull, 0u, 0u, 1048576ull, 256u}},
    {"64 MiB, lane_target 2304",
     {67108864ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 2304u, 0u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 1366ull, 1366ull, 0ull, 0u, 0ull, 128u, 87424ull, 0u, 0u, 1048576ull, 171u}},
    {"1 GiB",
     {1073741824ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 1986ull, 1986ull, 0ull, 0u, 0ull, 128u, 127104ull, 0u, 0u, 1048576ull, 249u}},
    {"1 GiB, lane_bytes 768 (taken)",
     {1073741824ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 768u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 23894ull, 19797ull, 384ull, 1u, 24576ull, 128u, 1529216ull, 0u, 0u, 1048576ull, 256u}},
    {"1 GiB, lane_bytes 1152 (taken)",
     {1073741824ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 1152u, 4, 1},
     {true, 8, 1152u, 32u, 3u, 73728ull, 18661ull, 12515ull, 384ull, 1u, 24576ull, 128u, 1194304ull, 0u, 0u, 1048576ull, 256u}},
    {"1 GiB, lane_bytes 800 (ignored)",
     {1073741824ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 800u, 4, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 1986ull, 1986ull, 0ull, 0u, 0ull, 128u, 127104ull, 0u, 0u, 1048576ull, 249u}},
    {"1 MiB + 5, lane_bytes 768 (taken)",
     {1048581ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 768u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 22ull, 22ull, 0ull, 0u, 0ull, 128u, 1408ull, 0u, 0u, 1048576ull, 3u}},
    {"1 MiB + 5, lane_bytes 65664 (ignored: over kLineLaneMax)",
     {1048581ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 65664u, 4, 1},
     {true, 8, 384u, 32u, 1u, 24576ull, 43ull, 43ull, 0ull, 0u, 0ull, 128u, 2752ull, 0u, 0u, 1048576ull, 6u}},
    {"1 GiB, regions_per_slot 2",
     {1073741824ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 0, false, 2, 8448u, 0u, 4, 1},
     {true, 8, 4224u, 32u, 11u, 270336ull, 3972ull, 3972ull, 0ull, 0u, 0ull, 128u, 254208ull, 0u, 0u, 1048576ull, 256u}},
    {"1 GiB, stitch_cus 32, split",
     {1073741824ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 32, true, 1, 8448u, 0u, 4, 1},
     {true, 8, 9600u, 32u, 25u, 614400ull, 1748ull, 1748ull, 0ull, 0u, 0ull, 128u, 111872ull, 0u, 0u, 1048576ull, 219u}},
    {"1 GiB, stitch_cus 32, one stream",
     {1073741824ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, true, 0, 8, 256, 32, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 8448u, 32u, 22u, 540672ull, 1986ull, 1986ull, 0ull, 0u, 0ull, 128u, 127104ull, 0u, 0u, 1048576ull, 249u}},
    {"32 MiB dense",
     {33554432ull, 1048576ull, 1048576ull, 0u, 49535u, true, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {false, 8, 432u, 432u, 5u, 27648ull, 1214ull, 1214ull, 0ull, 0u, 0ull, 27648u, 77696ull, 0u, 0u, 1048576ull, 152u}},
    {"64 MiB, discriminator 3",
     {67108864ull, 1048576ull, 1048576ull, 0u, 3u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 1366ull, 1366ull, 0ull, 0u, 0ull, 49152u, 87424ull, 0u, 0u, 1048576ull, 171u}},
    {"64 MiB, discriminator 2^32 - 1",
     {67108864ull, 1048576ull, 1048576ull, 0u, 4294967295u, false, false, true, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {true, 8, 768u, 32u, 2u, 49152ull, 1366ull, 1366ull, 0ull, 0u, 0ull, 64u, 87424ull, 0u, 0u, 1048576ull, 171u}},
    {"64 MiB rows, cfg 0",
     {67108864ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, false, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {false, 8, 528u, 32u, 6u, 33792ull, 1986ull, 1986ull, 0ull, 0u, 0ull, 128u, 127104ull, 0u, 0u, 1048576ull, 249u}},
    {"64 MiB rows, cfg 1",
     {67108864ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, false, 1, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {false, 12, 336u, 32u, 8u, 21504ull, 3121ull, 3121ull, 0ull, 0u, 0ull, 128u, 199744ull, 0u, 0u, 1048576ull, 256u}},
    {"64 MiB rows, cfg 2",
     {67108864ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, false, 2, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {false, 16, 240u, 32u, 6u, 15360ull, 4370ull, 4370ull, 0ull, 0u, 0ull, 128u, 279680ull, 0u, 0u, 1048576ull, 256u}},
    {"8 GiB rows, cfg 0",
     {8589934592ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, false, 0, 8, 256, 0, false, 1, 8448u, 0u, 4, 1},
     {false, 8, 32784u, 32u, 342u, 2098176ull, 4095ull, 4095ull, 0ull, 0u, 0ull, 256u, 262080ull, 0u, 0u, 1048576ull, 256u}},
    {"64 MiB rows, lane_bytes 336 (taken)",
     {67108864ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, false, 0, 8, 256, 0, false, 1, 8448u, 336u, 4, 1},
     {false, 8, 336u, 32u, 4u, 21504ull, 3121ull, 3121ull, 0ull, 0u, 0ull, 128u, 199744ull, 0u, 0u, 1048576ull, 256u}},
    {"64 MiB rows, lane_bytes 384 (ignored)",
     {67108864ull, 1048576ull, 1048576ull, 0u, 49535u, false, false, false, 0, 8, 256, 0, false, 1, 8448u, 384u, 4, 1},
     {false, 8, 528u, 32u, 6u, 33792ull, 1986ull, 1986ull, 0ull, 0u, 0ull, 128u, 127104ull, 0u, 0u, 1048576ull, 249u}},
};

static long bad = 0;

#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      if (++bad <= 20) {                     \
        printf("FAIL %s: ", #cond);          \
        printf(__VA_ARGS__);                 \
        printf("\n");                        \
      }                                      \
    }                                        \
  } while (0)

#define FIELD(f)                                                                              \
  CHECK(got.f == want.f, "row \"%s\": " #f " = %llu, recorded %llu", name, (unsigned long long)got.f, \
        (unsigned long long)want.f)

static void check_row(const char* name, const ScanGeom& got, const ScanGeom& want) {
  FIELD(line); FIELD(W); FIELD(S); FIELD(LS); FIELD(batches);
  FIELD(region_bytes); FIELD(nregions); FIELD(nbig); FIELD(S2); FIELD(batches2); FIELD(region_bytes2);
  FIELD(rcap); FIELD(nlanes); FIELD(delta); FIELD(shift0); FIELD(grid_P); FIELD(grid);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static void check_invariants(const ScanGeomIn& in, const ScanGeom& g) {
  const unsigned long long len = in.len, delta = in.delta;
  const uint64_t span = in.len + in.delta;
  const uint64_t ncu_scan = (uint64_t)(in.ncu - (in.split ? in.stitch_cus : 0));
  CHECK(g.line, "len %llu delta %llu", len, delta);
  CHECK(g.S % 384 == 0 && g.S >= 384 && g.S <= dsx::kLineLaneMax, "S %u (len %llu)", g.S, len);
  CHECK(g.batches == g.S / 384, "batches %u S %u", g.batches, g.S);
  CHECK(g.region_bytes == 64ull * g.S, "region_bytes %llu", (unsigned long long)g.region_bytes);
  if (g.S2 != 0) {
    CHECK(g.S2 % 384 == 0 && g.S2 < g.S, "S2 %llu S %u", (unsigned long long)g.S2, g.S);
    CHECK(g.batches2 == g.S2 / 384 && g.region_bytes2 == 64 * g.S2, "batches2 %u", g.batches2);
  } else {
    CHECK(g.nbig == g.nregions && g.region_bytes2 == 0 && g.batches2 == 0, "one size (len %llu)", len);
  }
  // the regions tile the span: the last one ends at or past it, and begins before it
  CHECK(g.nregions >= 1 && g.nbig <= g.nregions && g.nregions < (1ull << 32), "nregions %llu nbig %llu",
        (unsigned long long)g.nregions, (unsigned long long)g.nbig);
  const uint64_t small = g.nregions - g.nbig;
  const uint64_t covered = g.nbig * g.region_bytes + small * g.region_bytes2;
  const uint64_t last = small ? g.region_bytes2 : g.region_bytes;
  CHECK(covered >= span && covered - last < span, "covered %llu span %llu (len %llu delta %llu)",
        (unsigned long long)covered, (unsigned long long)span, len, delta);
  CHECK(g.nlanes == 64 * g.nregions, "nlanes %llu", (unsigned long long)g.nlanes);
  CHECK(g.rcap % 64 == 0 && g.rcap >= 64 && g.rcap <= 64 * g.S, "rcap %u S %u", g.rcap, g.S);
  CHECK(g.shift0 % 16 == 0 && g.shift0 < 256, "shift0 %u (halo %llu delta %llu)", g.shift0,
        (unsigned long long)in.halo, delta);
  CHECK(g.delta == in.delta && g.grid_P == in.P - in.delta, "grid_P %llu", (unsigned long long)g.grid_P);
  CHECK(g.grid >= 1 && g.grid <= ncu_scan, "grid %u", g.grid);
}

int main() {
  // a. the recorded rows
  const int nrows = (int)(sizeof kRows / sizeof kRows[0]);
  for (const Row& r : kRows) check_row(r.name, scan_geom(r.in), r.out);

  // b. invariants of the line scan
  const int kSweep = 4000;
  const int splits[3] = {0, 3, 4};
  const uint32_t targets[3] = {384, 2304, 8448};
  for (int n = 0; n < kSweep; ++n) {
    ScanGeomIn in;
    in.discriminator = 49535;
    // lengths of every magnitude up to 8 GiB, not only the large ones
    const uint64_t top = 1ull << (1 + rng() % 33);
    in.len = 1 + rng() % top;
    in.delta = (uint32_t)(rng() % 128);
    in.P = in.delta + rng() % (1ull << 40);
    in.halo = rng() % 2 ? in.P : rng() % 512;
    in.tail_split = splits[rng() % 3];
    in.lane_target = targets[rng() % 3];
    in.regions_per_slot = 1 + (int)(rng() % 2);
    check_invariants(in, scan_geom(in));
  }
  for (const Row& r : kRows)
    if (r.out.line) check_invariants(r.in, scan_geom(r.in));

  // c. the one-trip / two-trip rule at the defaults
  const uint64_t lanes = 256ull * 8 * 64;
  int nrule = 0;
  auto rule = [&](uint64_t len, uint32_t delta) {
    ScanGeomIn in;
    in.discriminator = 49535;
    in.len = len;
    in.delta = delta;
    in.P = in.halo = 1 << 20;
    const uint32_t want = len + delta > 384 * lanes ? 768u : 384u;
    const ScanGeom g = scan_geom(in);
    CHECK(g.S == want, "len %llu delta %u: S %u, rule %u", (unsigned long long)len, delta, g.S, want);
    ++nrule;
  };
  const uint32_t deltas[4] = {0, 1, 73, 127};
  for (uint32_t d : deltas) {
    const uint64_t lens[] = {1, 48, 383, 384, 384 * lanes - 128, 384 * lanes - d - 1, 384 * lanes - d,
                             384 * lanes - d + 1, 384 * lanes, 384 * lanes + 1, 576 * lanes,
                             768 * lanes - d - 1, 768 * lanes - d};
    for (uint64_t len : lens) rule(len, d);
  }
  for (int n = 0; n < 2000; ++n) {
    const uint32_t d = (uint32_t)(rng() % 128);
    rule(1 + rng() % (768 * lanes - d), d);
  }

  if (bad) {
    printf("scan geometry model: %ld checks failed\n", bad);
    return 1;
  }
  printf("scan geometry model ok: %d rows, %d sweep pieces, %d rule points\n", nrows, kSweep, nrule);
  return 0;
}
