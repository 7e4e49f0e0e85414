// dsx_many_plan.h -- the plan of a many-blob cut call as a pure function: how
// the blobs of one packed buffer are dealt to scan launches.
// Integer arithmetic only, no HIP: dsx_cut_device_many (dsx_engine.cpp) runs
// the items in order, and tests/test_many_host.py runs the function on the CPU
// (tests/many_plan_model.cpp).
#ifndef DSX_MANY_PLAN_H_
#define DSX_MANY_PLAN_H_
#include <stdint.h>

#include <vector>

namespace dsx_host {

// One work item: the consecutive blobs [b0, b1) and their bytes [start, end).
//   single: exactly one of the blobs is not empty (blob `big`) and takes the
//           one-blob path on its own;
//   group:  every blob is shorter than big_blob and the bytes are at most
//           group_bytes: one scan launch and one batched walk.
// Items tile the blob list in order.  A run of empty blobs joins the item
// before it (the first run: the item after it), so it never makes an item of
// its own unless every blob is empty; an item of no bytes launches nothing.
struct ManyItem {
  uint64_t b0 = 0, b1 = 0;
  uint64_t start = 0, end = 0;
  uint64_t big = 0;  // single: the blob that is not empty
  bool single = false;
};

// blob_ends: non-decreasing (the caller checked).  big_blob > 0, group_bytes > 0.
// A blob of more than group_bytes cannot share a launch with anything and no
// launch may hold it, so it is single whatever big_blob says.
inline std::vector<ManyItem> many_plan(const uint64_t* blob_ends, uint64_t nblobs,
                                       uint64_t big_blob, uint64_t group_bytes) {
  std::vector<ManyItem> items;
  bool open = false;  // the last item is a group that may still take blobs
  uint64_t lead = 0;  // empty blobs before the first item
  uint64_t B0 = 0;
  for (uint64_t i = 0; i < nblobs; ++i) {
    const uint64_t B1 = blob_ends[i], n = B1 - B0;
    if (n == 0) {
      if (items.empty()) ++lead;
      else items.back().b1 = i + 1;
      continue;
    }
    const bool single = n >= big_blob || n > group_bytes;
    if (!single && open && B1 - items.back().start <= group_bytes) {
      items.back().b1 = i + 1;
      items.back().end = B1;
    } else {
      ManyItem it;
      it.b0 = items.empty() ? i - lead : i;
      it.b1 = i + 1;
      it.start = B0;
      it.end = B1;
      it.big = i;
      it.single = single;
      items.push_back(it);
      open = !single;
    }
    B0 = B1;
  }
  if (items.empty() && nblobs) {  // every blob is empty
    ManyItem it;
    it.b1 = nblobs;
    items.push_back(it);
  }
  return items;
}

// The runs of a group's blobs that one workgroup of the batched walk takes:
// consecutive blobs [r.b0, r.b1) whose bytes span at most `span` (a longer
// blob is a run of its own) and that are at most `max_blobs`.
struct ManyRun {
  uint32_t b0, b1;
};
inline void many_runs(const uint64_t* blob_ends, uint64_t b0, uint64_t b1, uint64_t span,
                      uint32_t max_blobs, std::vector<ManyRun>* out) {
  out->clear();
  uint64_t r0 = b0, lo = b0 ? blob_ends[b0 - 1] : 0;
  for (uint64_t i = b0; i < b1; ++i) {
    if (i > r0 && (blob_ends[i] - lo > span || i - r0 >= max_blobs)) {
      out->push_back(ManyRun{(uint32_t)r0, (uint32_t)i});
      r0 = i;
      lo = blob_ends[i - 1];
    }
  }
  if (b1 > r0) out->push_back(ManyRun{(uint32_t)r0, (uint32_t)b1});
}

}  // namespace dsx_host
#endif  // DSX_MANY_PLAN_H_
