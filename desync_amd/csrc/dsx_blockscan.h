// dsx_blockscan.h -- the block-scan pattern of the chunk store, the range read
// and the many-blob cut (dsx_store.hip, dsx_read.hip, dsx_many.hip): mark the
// items you want, scan the marks into ranks and offsets, place the items at
// them.  The pieces, one definition each:
//   wave_*                    a scan and three reductions over a wave's lanes;
//   block_scan                every lane's exclusive prefix inside its workgroup
//                             and the workgroup's total, one or two words a lane;
//   block_totals_to           the workgroup's totals to blk[] (a select kernel
//                             needs no more: the array scan orders the workgroups);
//   block_array_scan_kernel   one workgroup turns blk[] into its exclusive prefix
//                             sums, in passes with a carry.
// All sums are of unsigned integers: the results do not depend on the order the
// waves' totals are added in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace dsx {

typedef unsigned long long u64;

// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ u64 wave_scan(u64 v) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= (uint32_t)o) v += t;
  }
  return v;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // (lane 0 holds the wave's sum)
}

__device__ __forceinline__ u64 wave_min(u64 v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = std::min<u64>(v, __shfl_down(v, o, 64));
  return v;  // (lane 0 holds the wave's minimum)
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = std::max<u64>(v, __shfl_down(v, o, 64));
  return v;  // (lane 0 holds the wave's maximum)
}

// Over a workgroup of NT threads, every thread calling: before[k] = the sum of
// v[k] over the lanes in front of this one, total[k] = over all of them.  Ends
// behind a barrier; a caller that calls it again puts a __syncthreads() between
// the calls (the next call writes the wave totals again).
template <int NT, int W>
__device__ __forceinline__ void block_scan(const u64 (&v)[W], u64 (&before)[W], u64 (&total)[W]) {
  __shared__ u64 s_wave[W][NT / 64];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  u64 incl[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    incl[k] = wave_scan(v[k]);
    if (lane == 63) s_wave[k][wave] = incl[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < W; ++k) {
    u64 off = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
      const u64 t = s_wave[k][w];
      off += (uint32_t)w < wave ? t : 0ull;
      all += t;
    }
    before[k] = off + incl[k] - v[k];
    total[k] = all;
  }
}

// wave_tot[k]: a wave's k-th total, held by its lane 0 (as wave_sum and a ballot
// leave it).  Thread 0 writes the workgroup's W totals to blk[W blockIdx.x ..].
template <int NT, int W>
__device__ __forceinline__ void block_totals_to(const u64 (&wave_tot)[W], u64* blk) {
  __shared__ u64 s_wave[W][NT / 64];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < W; ++k) s_wave[k][threadIdx.x >> 6] = wave_tot[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      u64 all = 0;
#pragma unroll
      for (int w = 0; w < NT / 64; ++w) all += s_wave[k][w];
      blk[W * (u64)blockIdx.x + k] = all;
    }
  }
}

constexpr int kArrayScanThreads = 256;

// One workgroup: the W-word elements blk[W j ..], j < nblk, become their
// exclusive prefix sums, kArrayScanThreads elements a pass with a carry between
// passes; total (may be null) receives the W sums.
template <int W>
__global__ __launch_bounds__(kArrayScanThreads) void block_array_scan_kernel(u64* blk, u64 nblk,
                                                                              u64* total) {
  u64 carry[W] = {};
  for (u64 base = 0; base < nblk; base += kArrayScanThreads) {
    const u64 j = base + threadIdx.x;
    u64 v[W], before[W], all[W];
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = j < nblk ? blk[W * j + k] : 0;
    block_scan<kArrayScanThreads, W>(v, before, all);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if (j < nblk) blk[W * j + k] = carry[k] + before[k];
      carry[k] += all[k];
    }
    __syncthreads();  // (the next pass writes the wave totals again)
  }
  if (total && threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < W; ++k) total[k] = carry[k];
  }
}

}  // namespace dsx
