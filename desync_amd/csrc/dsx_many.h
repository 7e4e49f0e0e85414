// dsx_many.h -- device structures of the many-blob cut (dsx_many.hip) shared
// with the host engine (dsx_engine.cpp).  DESIGN.md 4.9.
#pragma once
#include <stdint.h>

#include "dsx_stitch.h"

namespace dsx {

// Per-blob state of one dsx_cut_device_many call.  Blob i is [B0, B1) =
// [ends[i-1], ends[i]) of the packed buffer (ends[-1] = 0); its cuts are
// stage[B0 / min + i ..), cnt[i] of them: blob i has at most (B1 - B0) / min + 1
// cuts, so the slots of different blobs are disjoint.
struct ManyBlobs {
  const uint64_t* ends;  // [nblobs] device copy of blob_ends
  uint64_t* stage;       // [len / min + nblobs]
  uint32_t* cnt;         // [nblobs] (zeroed at the start of the call)
  uint32_t* flag;        // [nblobs] 1: the batched walk could not hold the blob (zeroed likewise)
  uint64_t nblobs;
  uint64_t min, max;
};

struct ManyRunDev {
  uint32_t b0, b1;  // blobs [b0, b1) of one workgroup
};

struct ManyWalkArgs {
  ManyBlobs mb;
  PieceCands pc;           // the group's scan
  const ManyRunDev* runs;  // [gridDim.x]
  uint32_t lds_cap;        // candidates a workgroup stages (<= kManyLdsCap)
  uint32_t pad;
};

struct ManyFinishArgs {
  ManyBlobs mb;
  uint64_t* first;  // [nblobs + 1] exclusive scan of cnt
  uint64_t* res;    // {total cuts, flagged blobs}
  uint64_t* out;    // contiguous cut list (device)
};

constexpr uint32_t kManyLdsCap = 8192;  // = kWalkLdsCap (dsx_engine.h)
constexpr int kManyWalkThreads = 256;
constexpr int kManyScanThreads = 1024;
constexpr int kManyGatherThreads = 256;

}  // namespace dsx
