// dsx_inplace_plan.h -- the schedule of an in-place assembly as a pure
// function ("In place"): which launches of the gather kernel,
// over which segment tables, turn a buffer that holds an old version into the
// target without a second buffer.  Integer arithmetic only, no HIP:
// dsx_assemble_inplace (dsx_assemble.hip) uploads the tables and runs the
// launches in order, dsx_inplace_plan (dsx_plan.cpp) hands them to callers
// without a GPU, and tests/inplace_replay.cpp replays them under a host
// sanitizer.
//
// The destination is cut into windows on the gather's tile grid of the
// buffer: byte x lies in window (x + skew) / window.  Windows that hold
// something to write are visited in one direction, ascending or descending.
// Before window r is visited,
//   * every old byte of r and of the windows still to come is intact, as is
//     every byte of a window nothing writes and every byte at or beyond
//     new_len (no launch ever writes those);
//   * every old byte of a window already visited that a piece of r or of a
//     window still to come reads lies in the stash.
// Window r then issues at most two launches, in stream order:
//   A (save)   gathers into freshly allocated stash ranges the old bytes of
//              window r that a piece of r or of a later window reads: it reads
//              window r of the buffer only and writes the stash only;
//   B (write)  gathers r's pieces into the buffer: it writes window r only and
//              reads the stash, intact bytes outside window r, the seeds, the
//              store and zeros.
// Two launches suffice because the kernel's only hazard is a launch that reads
// what it writes: A moves every byte B would both read and destroy out of the
// way first, and everything a later window needs with it.  A stash range is
// freed after the last window that reads it; each old byte is saved at most
// once, so the stash never holds more than have_len bytes.
//
// The safety argument is this range disjointness alone: assemble_kernel reads
// no byte outside a piece's source range (dsx_assemble.hip, "no byte outside
// a source range is ever read") and writes no byte outside its destination,
// so a launch whose read ranges and write ranges are disjoint cannot destroy
// what it, or a later launch, still has to read.
#ifndef DSX_INPLACE_PLAN_H_
#define DSX_INPLACE_PLAN_H_
#include <stdint.h>

#include <algorithm>
#include <queue>
#include <utility>
#include <vector>

#include "../../include/dsx.h"

namespace dsx_host {

struct InplacePlan {
  std::vector<dsx_inplace_launch_t> launches;
  std::vector<dsx_plan_seg_t> segs;  // every launch's table, one behind the other
  dsx_inplace_totals_t totals{};
  const char* why = nullptr;  // DSX_E_INVAL: what was wrong ...
  uint64_t bad_seg = 0;       // ... and in which segment (UINT64_MAX: none)
};

namespace inplace_detail {

typedef uint64_t u64;

struct Piece {  // bytes to write, cut at window edges
  u64 dst, bytes, src_off;
  int32_t source;
};
struct Win {  // a window that holds pieces [p0, p1)
  u64 r, p0, p1;
};
struct Need {  // old bytes [x0, x1) of one window, read last by the window visited at step `last`
  u64 x0, x1, last;
};
struct Frag {  // old bytes [x0, x1) lie in the stash at off
  u64 x0, x1, off;
};

struct Builder {
  u64 have_len, new_len, skew, window;
  std::vector<Piece> pieces;
  std::vector<Win> wins;

  u64 win_of(u64 x) const { return (x + skew) / window; }
  // the end of the window x lies in (lengths and window are at most 2^62)
  u64 win_end(u64 x) const { return (win_of(x) + 1) * window - skew; }
  // index into wins of window r, or -1: nothing writes it
  int64_t find(u64 r) const {
    size_t lo = 0, hi = wins.size();
    while (lo < hi) {
      const size_t m = (lo + hi) / 2;
      if (wins[m].r < r) lo = m + 1;
      else hi = m;
    }
    return lo < wins.size() && wins[lo].r == r ? (int64_t)lo : -1;
  }

  // Calls fn(vi, x0, x1, d) for each part [x0, x1) of a SELF piece's source,
  // cut at window edges and at new_len; d is the part's destination.  vi is the
  // index of the window the part has to come out of the stash of, or -1 when
  // the part is read where it lies: beyond new_len, in a window nothing
  // writes, or in a window visited after the piece's own (index ri).
  template <class F>
  void parts(const Piece& p, u64 ri, bool desc, F&& fn) const {
    u64 x = p.src_off, d = p.dst;
    const u64 end = p.src_off + p.bytes;
    while (x < end) {
      u64 e = std::min(end, win_end(x));
      if (x < new_len) e = std::min(e, new_len);
      int64_t vi = -1;
      if (x < new_len) {
        vi = find(win_of(x));
        if (vi >= 0 && (desc ? (u64)vi < ri : (u64)vi > ri)) vi = -1;
      }
      fn(vi, x, e, d);
      d += e - x;
      x = e;
    }
  }

  // what each window has to save, merged, and the stash's peak
  void analyse(bool desc, std::vector<std::vector<Need>>* need, u64* peak, u64* saved) const {
    const size_t W = wins.size();
    need->assign(W, {});
    for (size_t ri = 0; ri < W; ++ri)
      for (u64 k = wins[ri].p0; k < wins[ri].p1; ++k) {
        if (pieces[k].source != DSX_SRC_SELF) continue;
        parts(pieces[k], ri, desc, [&](int64_t vi, u64 x0, u64 x1, u64) {
          if (vi >= 0) (*need)[vi].push_back(Need{x0, x1, (u64)(desc ? W - 1 - ri : ri)});
        });
      }
    std::vector<u64> freed(W, 0);
    *saved = 0;
    std::vector<Need> u;
    for (size_t vi = 0; vi < W; ++vi) {
      // the union of what is read, cut where the last reader changes (each byte
      // is freed after its own last reader): a sweep over the sorted starts
      // with the open reads in a heap, the latest reader on top
      std::vector<Need>& v = (*need)[vi];
      std::sort(v.begin(), v.end(), [](const Need& a, const Need& b) { return a.x0 < b.x0; });
      std::priority_queue<std::pair<u64, u64>> open;  // {last, x1}
      u.clear();
      size_t i = 0;
      u64 x = 0;
      while (i < v.size() || !open.empty()) {
        if (open.empty()) x = v[i].x0;
        for (; i < v.size() && v[i].x0 <= x; ++i) open.push({v[i].last, v[i].x1});
        while (!open.empty() && open.top().second <= x) open.pop();
        if (open.empty()) continue;
        u64 e = open.top().second;
        if (i < v.size()) e = std::min(e, v[i].x0);
        if (!u.empty() && u.back().x1 == x && u.back().last == open.top().first) u.back().x1 = e;
        else u.push_back(Need{x, e, open.top().first});
        x = e;
      }
      v = u;
      for (const Need& q : v) {
        freed[q.last] += q.x1 - q.x0;
        *saved += q.x1 - q.x0;
      }
    }
    u64 live = 0;
    *peak = 0;
    for (size_t s = 0; s < W; ++s) {
      const size_t i = desc ? W - 1 - s : s;
      for (const Need& q : (*need)[i]) live += q.x1 - q.x0;
      *peak = std::max(*peak, live);
      live -= freed[s];
    }
  }

  // the launches of one direction; the stash is exactly `peak` bytes
  void emit(bool desc, const std::vector<std::vector<Need>>& need, u64 peak, InplacePlan* out) const {
    const size_t W = wins.size();
    std::vector<std::pair<u64, u64>> holes;  // free stash ranges {off, len}, ascending
    if (peak) holes.push_back({0, peak});
    std::vector<std::vector<Frag>> frags(W);
    std::vector<std::vector<std::pair<u64, u64>>> free_at(W);
    auto seg = [](u64 dst, u64 bytes, int32_t source, u64 src_off) {
      dsx_plan_seg_t g{};
      g.dst_off = dst, g.bytes = bytes, g.src_off = src_off, g.source = source;
      g.seed_first = 0xFFFFFFFFu;
      return g;
    };
    for (size_t s = 0; s < W; ++s) {
      const size_t i = desc ? W - 1 - s : s;
      const Win& w = wins[i];
      // ---- A: save -----------------------------------------------------------
      if (!need[i].empty()) {
        dsx_inplace_launch_t a{};
        a.window = w.r, a.kind = DSX_INPLACE_SAVE, a.seg0 = out->segs.size();
        a.lo = UINT64_MAX;
        for (const Need& q : need[i]) {
          u64 x = q.x0;
          size_t h = 0;  // (the lowest holes first: the table ascends in dst_off)
          while (x < q.x1) {
            const u64 take = std::min(q.x1 - x, holes[h].second);
            const u64 off = holes[h].first;
            out->segs.push_back(seg(off, take, DSX_SRC_SELF, x));
            frags[i].push_back(Frag{x, x + take, off});
            free_at[q.last].push_back({off, take});
            a.lo = std::min(a.lo, off), a.hi = std::max(a.hi, off + take);
            holes[h].first += take, holes[h].second -= take;
            if (!holes[h].second) ++h;
            x += take;
          }
          holes.erase(holes.begin(), holes.begin() + h);
        }
        a.nsegs = out->segs.size() - a.seg0;
        out->launches.push_back(a);
      }
      // ---- B: write ----------------------------------------------------------
      dsx_inplace_launch_t b{};
      b.window = w.r, b.kind = DSX_INPLACE_WRITE, b.seg0 = out->segs.size();
      b.lo = pieces[w.p0].dst, b.hi = pieces[w.p1 - 1].dst + pieces[w.p1 - 1].bytes;
      for (u64 k = w.p0; k < w.p1; ++k) {
        const Piece& p = pieces[k];
        if (p.source != DSX_SRC_SELF) {
          out->segs.push_back(seg(p.dst, p.bytes, p.source, p.src_off));
          continue;
        }
        parts(p, i, desc, [&](int64_t vi, u64 x0, u64 x1, u64 d) {
          if (vi < 0) {
            out->segs.push_back(seg(d, x1 - x0, DSX_SRC_SELF, x0));
            return;
          }
          const std::vector<Frag>& f = frags[vi];
          size_t j = std::upper_bound(f.begin(), f.end(), x0,
                                      [](u64 x, const Frag& q) { return x < q.x1; }) - f.begin();
          for (u64 x = x0; x < x1; ++j) {  // (the fragments cover [x0, x1): analyse() merged it in)
            const u64 e = std::min(x1, f[j].x1);
            out->segs.push_back(seg(d + (x - x0), e - x, DSX_SRC_STASH, f[j].off + (x - f[j].x0)));
            x = e;
          }
        });
      }
      b.nsegs = out->segs.size() - b.seg0;
      out->launches.push_back(b);
      // ---- free what window r read last --------------------------------------
      for (const auto& fr : free_at[s]) {
        auto it = std::lower_bound(holes.begin(), holes.end(), fr);
        it = holes.insert(it, fr);
        if (it + 1 != holes.end() && it->first + it->second == (it + 1)->first) {
          it->second += (it + 1)->second;
          holes.erase(it + 1);
        }
        if (it != holes.begin() && (it - 1)->first + (it - 1)->second == it->first) {
          (it - 1)->second += it->second;
          holes.erase(it);
        }
      }
    }
  }
};

}  // namespace inplace_detail

// The schedule.  Returns DSX_OK, DSX_E_INVAL (out->why says what, out->bad_seg
// where) or DSX_E_CAPACITY (the chosen direction's peak exceeds stash_cap:
// out->totals.stash_peak is what it needs, and no launch is listed).  Throws
// std::bad_alloc.
inline int inplace_plan(const dsx_plan_seg_t* segs, uint64_t nsegs, const uint64_t* ends, uint64_t n,
                        const uint8_t* keep, uint64_t have_len, uint64_t new_len, uint64_t skew,
                        uint64_t tile, uint64_t window, uint64_t stash_cap, uint32_t flags,
                        InplacePlan* out) {
  using namespace inplace_detail;
  *out = InplacePlan{};
  out->bad_seg = UINT64_MAX;
  auto bad = [&](uint64_t i, const char* why) {
    out->bad_seg = i, out->why = why;
    return DSX_E_INVAL;
  };
  const uint32_t f_dir = DSX_INPLACE_ASCENDING | DSX_INPLACE_DESCENDING;
  if ((flags & ~f_dir) != 0) return bad(UINT64_MAX, "unknown flag bits");
  if ((flags & f_dir) == f_dir) return bad(UINT64_MAX, "both directions are forced");
  if ((nsegs && !segs) || (n && !ends)) return bad(UINT64_MAX, "a NULL array");
  if (!tile || !window || window % tile != 0) return bad(UINT64_MAX, "window is no positive multiple of tile");
  if (skew >= tile) return bad(UINT64_MAX, "skew is not below tile");
  if (n > 0xFFFFFFF0ull) return bad(UINT64_MAX, "too many chunks");
  const uint64_t kMax = 1ull << 62;
  if (new_len > kMax || have_len > kMax || window > kMax) return bad(UINT64_MAX, "a length beyond 2^62");
  for (u64 i = 0, prev = 0; i < n; ++i) {
    if (ends[i] < prev || ends[i] > new_len) return bad(UINT64_MAX, "chunk ends decrease or exceed new_len");
    prev = ends[i];
  }

  Builder b;
  b.have_len = have_len, b.new_len = new_len, b.skew = skew, b.window = window;
  dsx_inplace_totals_t& t = out->totals;
  // ---- the pieces: segments without what is kept, cut at window edges ----------
  auto add = [&](u64 dst, u64 bytes, int32_t source, u64 src_off) {
    t.written_bytes += bytes;
    while (bytes) {
      const u64 take = std::min(bytes, b.win_end(dst) - dst);
      const u64 r = b.win_of(dst);
      if (b.wins.empty() || b.wins.back().r != r) b.wins.push_back(Win{r, b.pieces.size(), b.pieces.size()});
      b.pieces.push_back(Piece{dst, take, source == DSX_SRC_NULL ? 0 : src_off, source});
      b.wins.back().p1 = b.pieces.size();
      dst += take, src_off += take, bytes -= take;
    }
  };
  u64 prev_end = 0;
  for (u64 i = 0; i < nsegs; ++i) {
    const dsx_plan_seg_t& g = segs[i];
    if (g.dst_off < prev_end) return bad(i, "dst_off is below the end of the segment before it");
    if (g.bytes > new_len || g.dst_off > new_len - g.bytes) return bad(i, "dst_off + bytes is beyond new_len");
    if (g.source < DSX_SRC_SELF) return bad(i, "source is neither a seed, the null seed, the store nor the buffer");
    if ((u64)g.first + g.count > n) return bad(i, "first + count is beyond the chunks");
    const u64 c0 = g.first ? ends[g.first - 1] : 0;
    const u64 c1 = g.count ? ends[g.first + g.count - 1] : c0;
    if (g.count ? (g.dst_off != c0 || g.bytes != c1 - c0) : g.bytes != 0)
      return bad(i, "dst_off and bytes are not those of the chunks it names");
    if (g.source == DSX_SRC_SELF && (g.bytes > have_len || g.src_off > have_len - g.bytes))
      return bad(i, "src_off + bytes is beyond the old content");
    if (g.source != DSX_SRC_SELF && g.source != DSX_SRC_NULL && g.src_off > UINT64_MAX - g.bytes)
      return bad(i, "src_off + bytes overflows");
    prev_end = g.dst_off + g.bytes;
    const bool same = g.source == DSX_SRC_SELF && g.src_off == g.dst_off;
    if (!same && !keep) {
      add(g.dst_off, g.bytes, g.source, g.src_off);
      continue;
    }
    u64 run0 = c0, at = c0;  // the open run of chunks to write is [run0, at)
    for (u64 k = g.first; k < (u64)g.first + g.count; ++k) {
      const u64 e = ends[k];
      if (same || keep[k]) {
        if (at > run0) add(run0, at - run0, g.source, g.src_off + (run0 - c0));
        ++t.kept_chunks, t.kept_bytes += e - at;
        run0 = e;
      }
      at = e;
    }
    if (at > run0) add(run0, at - run0, g.source, g.src_off + (run0 - c0));
  }

  // ---- the direction ---------------------------------------------------------
  std::vector<std::vector<Need>> need[2];
  u64 peak[2] = {0, 0}, saved[2] = {0, 0};
  const bool want[2] = {(flags & DSX_INPLACE_DESCENDING) == 0, (flags & DSX_INPLACE_ASCENDING) == 0};
  for (int d = 0; d < 2; ++d)
    if (want[d]) b.analyse(d == 1, &need[d], &peak[d], &saved[d]);
  const int d = !want[0] ? 1 : !want[1] ? 0 : (peak[1] < peak[0] ? 1 : 0);
  t.direction = d ? DSX_INPLACE_DESCENDING : DSX_INPLACE_ASCENDING;
  t.stash_peak = peak[d];
  t.stash_bytes = saved[d];
  if (peak[d] > stash_cap) return DSX_E_CAPACITY;
  b.emit(d == 1, need[d], peak[d], out);
  t.windows = b.wins.size();
  t.launches = out->launches.size();
  t.segments = out->segs.size();
  return DSX_OK;
}

}  // namespace dsx_host
#endif  // DSX_INPLACE_PLAN_H_
