// dsx_many.hip -- the cut lists of many blobs packed in one buffer
// (dsx_cut_device_many).
//
// A group of blobs is scanned by one launch of the scan over its bytes
// (dsx_scan.hip, unchanged: a candidate whose window straddles a blob boundary
// lies in (B0, B0 + 47] and is never eligible, because the chain of the blob
// from B0 only tests positions above B0 + min >= B0 + 48).  Every blob
// boundary is a certain cut, so every blob's chain has a known entry: no
// speculation, no fixup, no repair.
//   many_walk_kernel    a workgroup stages the candidates of a run of
//                       consecutive blobs in LDS (as walk_kernel does for its
//                       segments); blobs of at most `min` bytes are one chunk
//                       and are written a lane each; every other blob is one
//                       chain walked by one wave (rel_step of dsx_chain.h with
//                       L = B1, entry B0).  Blob i's cuts go to its own slots
//                       of the staging list, their count to cnt[i].
//   many_scan_kernel    exclusive scan of cnt[] over the blobs (block_scan,
//                       dsx_blockscan.h): blob_first.
//   many_gather_kernel  staging list -> contiguous cut list.
#include <hip/hip_runtime.h>

#include "dsx_blockscan.h"
#include "dsx_chain.h"
#include "dsx_common.h"
#include "dsx_many.h"

namespace dsx {

__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
  return ((uint64_t)hi << 32) | lo;
}

// The host keeps a run's bytes below 2^30 (a longer blob takes the one-blob
// path), so positions relative to the run's start and a step of max (clamped
// to 2^30 as rel_chain does) fit 32 bits.
__global__ __launch_bounds__(kManyWalkThreads) void many_walk_kernel(ManyWalkArgs a) {
  constexpr int NT = kManyWalkThreads;
  constexpr uint32_t kWaves = NT / 64;
  __shared__ uint32_t cand[kManyLdsCap];
  __shared__ uint32_t s_off[kWalkMaxRegions + 1];
  __shared__ uint32_t s_wave[kWaves];
  const ManyBlobs& mb = a.mb;
  const PieceCands& pc = a.pc;
  const uint32_t b0 = __builtin_amdgcn_readfirstlane(a.runs[blockIdx.x].b0);
  const uint32_t b1 = __builtin_amdgcn_readfirstlane(a.runs[blockIdx.x].b1);
  if (b1 <= b0) return;
  const uint64_t lo = uniform64(b0 ? mb.ends[b0 - 1] : 0ull);
  const uint64_t hi = uniform64(mb.ends[b1 - 1]);

  // ---- the candidates in (lo, hi] into LDS, sorted (region order) ----
  const uint64_t r0 = lo <= pc.P ? 0 : pc_region_of(pc, lo - pc.P);
  uint64_t r1 = hi <= pc.P ? 0 : pc_region_of(pc, hi - pc.P - 1) + 1;  // exclusive
  if (r1 > pc.nregions) r1 = pc.nregions;
  const uint32_t nreg = r1 > r0 ? (uint32_t)(r1 - r0) : 0u;
  // the scan's lists overflowed, or the run does not fit: its chains are
  // flagged for the one-blob path, nothing is truncated
  bool dense = *pc.overflow != 0u || nreg > kWalkMaxRegions || hi - lo > (1ull << 30);
  uint32_t total = 0;
  if (!dense) {
    for (uint32_t b = 0; b < nreg; b += NT) {
      const uint32_t i = b + threadIdx.x;
      uint32_t c = 0;
      if (i < nreg) {
        c = pc.region_cnt[r0 + i];
        c = c < pc.region_cap ? c : pc.region_cap;
      }
      uint32_t part;
      const uint32_t ex = walk_block_scan<NT>(c, s_wave, &part);
      if (i < nreg) s_off[i] = total + ex;
      total += part;
    }
    if (threadIdx.x == 0) s_off[nreg] = total;
    __syncthreads();
    dense = total > a.lds_cap;
  }
  if (!dense) {
    for (uint32_t g = threadIdx.x; g < total; g += NT) {
      uint32_t l = 0, h = nreg;  // last r with s_off[r] <= g
      while (h - l > 1) {
        const uint32_t m = (l + h) >> 1;
        if (s_off[m] <= g) l = m; else h = m;
      }
      const uint64_t r = r0 + l;
      const uint64_t p = pc.P + pc_region_base(pc, r) +
                         pc.region_list[r * (uint64_t)pc.region_cap + (g - s_off[l])];
      // keep the array sorted: below-range -> 0, above-range -> UINT32_MAX
      cand[g] = p <= lo ? 0u : (p > hi ? 0xFFFFFFFFu : (uint32_t)(p - lo));
    }
  }
  __syncthreads();

  // ---- the blobs: 64 at a time per wave, a lane each ----
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), ln = threadIdx.x & 63;
  const uint32_t nb = b1 - b0;
  RelChain rc;
  rc.min = mb.min < (1ull << 30) ? (uint32_t)mb.min : (1u << 30);
  rc.max = mb.max < (1ull << 30) ? (uint32_t)mb.max : (1u << 30);
  rc.is_last = true;
  rc.undet_at = 0xFFFFFFFFu;
  // One source per wave for all its chains: the wave takes its blobs in
  // ascending order and a chain only looks forward, so the register window
  // moves forward through the candidates once.
  WaveLdsSrc src{cand, total, 0, lo, ln, 0};
  if (!dense) src.load();
  for (uint32_t t = wv * 64u; t < nb; t += kWaves * 64u) {
    const uint32_t i = b0 + t + ln;
    uint64_t B0 = 0, B1 = 0;
    bool chain = false;
    if (t + ln < nb) {
      B1 = mb.ends[i];
      B0 = i ? mb.ends[i - 1] : 0ull;
      const uint64_t n = B1 - B0;
      chain = n > mb.min;
      if (!chain && n) {  // chunker.go:215-217: one chunk, no candidate is looked at
        mb.stage[B0 / mb.min + i] = B1;
        mb.cnt[i] = 1u;
      }
    }
    uint64_t m = __ballot(chain);
    if (dense) {
      if (chain) mb.flag[i] = 1u;
      continue;
    }
    while (m) {  // one chain at a time, the whole wave on it
      const uint32_t l = (uint32_t)__builtin_ctzll(m);
      m &= m - 1;
      const uint64_t c0 = readlane64(B0, l), c1 = readlane64(B1, l);
      const uint32_t j = b0 + t + l;
      rc.L = (uint32_t)(c1 - lo);
      rc.PE = rc.L;
      rc.tail_at = (uint32_t)(c1 - mb.min - lo);  // (c1 - c0 > min)
      rc.lim_cap = rc.L;
      rc.end_at = rc.L;
      uint64_t* out = mb.stage + (c0 / mb.min + j);
      const uint32_t slots = (uint32_t)((c1 - c0) / mb.min) + 1u;
      uint32_t x = (uint32_t)(c0 - lo), n = 0;
      while (true) {
        uint32_t nx;
        if (x >= rc.tail_at) {
          if (x >= rc.end_at) break;
          nx = rc.L;  // chunker.go:215-217
        } else {
          nx = rel_step(x, src, rc);
        }
        if (ln == (n & 63u) && n < slots) out[n] = lo + nx;  // spread the stores over lanes
        ++n;
        x = nx;
      }
      if (ln == 0) {
        mb.cnt[j] = n <= slots ? n : 0u;
        if (n > slots) mb.flag[j] = 1u;  // (cannot happen: every chunk but the last is > min)
      }
    }
  }
}

// One workgroup: first[i] = cuts of the blobs before i, first[nblobs] and
// res[0] the total, res[1] the flagged blobs.
__global__ __launch_bounds__(kManyScanThreads) void many_scan_kernel(ManyFinishArgs a) {
  constexpr int NT = kManyScanThreads;
  __shared__ unsigned long long s_flag;
  const ManyBlobs& mb = a.mb;
  if (threadIdx.x == 0) s_flag = 0;
  uint64_t base = 0, nflag = 0;
  for (uint64_t b = 0; b < mb.nblobs; b += NT) {
    const uint64_t i = b + threadIdx.x;
    u64 v[1] = {0}, before[1], all[1];
    if (i < mb.nblobs) {
      v[0] = mb.cnt[i];
      nflag += mb.flag[i] ? 1u : 0u;
    }
    block_scan<NT, 1>(v, before, all);
    if (i < mb.nblobs) a.first[i] = base + before[0];
    base += all[0];
    __syncthreads();  // (the next pass writes the wave totals again)
  }
  if (nflag) atomicAdd(&s_flag, (unsigned long long)nflag);
  __syncthreads();
  if (threadIdx.x == 0) {
    a.first[mb.nblobs] = base;
    a.res[0] = base;
    a.res[1] = s_flag;
  }
}

// Blob i's cuts from its slots of the staging list to out[first[i] ..): a
// lane each for up to 4 cuts, the whole wave on every longer list in turn.
__global__ __launch_bounds__(kManyGatherThreads) void many_gather_kernel(ManyFinishArgs a) {
  const ManyBlobs& mb = a.mb;
  const uint64_t i = (uint64_t)blockIdx.x * kManyGatherThreads + threadIdx.x;
  const uint32_t ln = threadIdx.x & 63;
  uint32_t c = 0;
  uint64_t src = 0, dst = 0;  // element indices
  if (i < mb.nblobs) {
    c = mb.cnt[i];
    src = (i ? mb.ends[i - 1] : 0ull) / mb.min + i;
    dst = a.first[i];
  }
  if (c <= 4u)
    for (uint32_t k = 0; k < c; ++k) a.out[dst + k] = mb.stage[src + k];
  uint64_t m = __ballot(c > 4u);
  while (m) {
    const uint32_t l = (uint32_t)__builtin_ctzll(m);
    m &= m - 1;
    const uint64_t s = readlane64(src, l), d = readlane64(dst, l);
    const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)l);
    for (uint32_t k = ln; k < n; k += 64u) a.out[d + k] = mb.stage[s + k];
  }
}

}  // namespace dsx
