// The smallest piece that scanl_kernel scans with two region sizes under
// DSX_LANE_TARGET=768 DSX_TAIL_SPLIT=2 on a device of `ncu` compute units, from
// scan_geom() (desync_amd/csrc/dsx_scan_geom.h).  Built and run by
// tests/test_gpu_scan_linefetch.py:
//   g++ -std=c++17 -O1 -Wall -Werror -Iinclude -Idesync_amd/csrc tests/scan_two_size.cpp
// Prints "len S S2 nbig nregions" for a piece at a line-aligned pointer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "dsx_scan_geom.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  dsx_host::ScanGeomIn in;
  in.ncu = atoi(argv[1]);
  in.P = in.halo = 1ull << 30;
  in.discriminator = 65536;
  in.lane_target = 768;
  in.tail_split = 2;
  auto at = [&](uint64_t len) {
    in.len = len;
    return dsx_host::scan_geom(in);
  };
  // S2 != 0 is monotonic in len once S has reached the target: bisect
  uint64_t lo = 1, hi = 1ull << 32;
  if (at(hi).S2 == 0) return 3;
  while (lo + 1 < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (at(mid).S2 != 0) hi = mid;
    else lo = mid;
  }
  const dsx_host::ScanGeom g = at(hi);
  if (g.S2 == 0 || at(hi - 1).S2 != 0 || !g.line) return 4;
  printf("%llu %u %llu %llu %llu\n", (unsigned long long)hi, g.S, (unsigned long long)g.S2,
         (unsigned long long)g.nbig, (unsigned long long)g.nregions);
  return 0;
}
