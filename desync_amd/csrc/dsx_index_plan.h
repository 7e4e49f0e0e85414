// dsx_index_plan.h -- the plans of the file pipeline as pure functions: the
// window geometry of run_index and run_ids (dsx_index.cpp), the pieces the
// readers fetch, the GPU's shares during the read, and who hashes which chunk
// of the last window.  Arithmetic only, no HIP and no context:
// run_index executes index_schedule and run_ids executes ids_schedule as they
// stand here, the diagnostic library exports both (dsx_diag_index_schedule,
// dsx_diag_ids_schedule) and tests/index_plan_model.cpp sweeps them on the CPU
// under the host sanitizers.
#ifndef DSX_INDEX_PLAN_H_
#define DSX_INDEX_PLAN_H_
#include <stdint.h>

#include <algorithm>
#include <vector>
#if DSX_DIAG
#include <cstdlib>
#endif

#include "dsx_common.h"

namespace dsx_host {

// the side streams of the file pipeline (dsx_ctx::idx_side): at most this
// many GPU shares of a call during its read
constexpr int kIdxSide = 4;

// bytes per scan + stitch launch: each stitch publishes the chain position
// (dsx_progress), so 32 per GiB, make.go:138's pb.Set per chunk in steps of
// 32 MiB; the GPU work per step (~40 us) is far below its PCIe time (~1 ms)
constexpr uint64_t kScanStep = 32ull << 20;

// the read-time model of the shares (plan_shares) and of run_ids's budget
constexpr double kShareNsPerByte = 45.0;  // digest_pc_kernel, one lane, beside the read's scans (37-40, r06an)
constexpr double kReadBytesPerNs = 45.0;  // page cache -> HBM through the pinned slots (dsx_cut_fd, ~42 GiB/s)
constexpr uint64_t kFineTail = 32ull << 20;  // the call's last bytes in smaller pieces
constexpr uint64_t kFineDiv = 4;             // of piece / kFineDiv bytes

// Pieces [0, len): `piece` bytes each up to fine_from (a multiple of piece),
// `fine` bytes from there on (none when fine_from >= len).
struct PieceMap {
  uint64_t len, piece, fine_from, fine, kf, np;
  PieceMap(uint64_t n, uint64_t pc, uint64_t ff = UINT64_MAX, uint64_t fn = 0)
      : len(n), piece(pc), fine_from(fn && ff < n ? ff : UINT64_MAX), fine(fn ? fn : pc),
        kf(fine_from < n ? fine_from / pc : (n + pc - 1) / pc),
        np(kf + (fine_from < n ? (n - fine_from + fine - 1) / fine : 0)) {}
  uint64_t off(uint64_t k) const { return k < kf ? k * piece : fine_from + (k - kf) * fine; }
  uint64_t size(uint64_t k) const { return std::min(k < kf ? piece : fine, len - off(k)); }
};

// The windows of a call over `len` bytes: pieces (pinned slots of at most
// `slot` bytes, whole pages) tile the windows exactly; a window keeps `pre`
// bytes of its predecessor in front (at least `keep`, line aligned) and is at
// least 2 pre long.  run_index keeps max + 64 bytes (the unfinished chunk and
// the scan's warm-up), run_ids the list's longest chunk.  At least one piece
// and one window, whatever len (a list of empty chunks has 0 bytes).
struct WindowGeom {
  uint64_t pre, piece, W, nwin;
};
inline WindowGeom window_geom(uint64_t len, uint64_t keep, uint64_t slot, uint64_t window) {
  WindowGeom g;
  g.pre = (keep + dsx::kLine - 1) / dsx::kLine * dsx::kLine;
  g.piece = std::min<uint64_t>(slot, std::max<uint64_t>(len, 4096));
  g.piece = (g.piece + 4095) & ~4095ull;
  g.W = std::max<uint64_t>(window, 2 * g.pre);
  g.W = (g.W + g.piece - 1) / g.piece * g.piece;
  if (g.W >= len) g.W = std::max<uint64_t>(g.piece, (len + g.piece - 1) / g.piece * g.piece);  // one window
  g.nwin = std::max<uint64_t>(1, (len + g.W - 1) / g.W);
  return g;
}

// run_index's geometry: window_geom with max + 64 bytes kept.  The file's last
// kFineTail bytes (in its last window) are read, copied and scanned in pieces
// of piece / kFineDiv when the tail feeder runs (`feeds`): it then sees the
// long chunks of the call's last piece, the host's last batch, a few MB
// sooner.  (Smaller pieces throughout slow the read: 8 MiB slots, 28 against
// 45 GiB/s for dsx_cut_fd, profiles/r06ad.)
struct IndexGeom : WindowGeom {
  uint64_t fine, fine_from = UINT64_MAX;
  IndexGeom(uint64_t len, uint64_t max_chunk, uint64_t slot, uint64_t window, bool feeds)
      : WindowGeom(window_geom(len, max_chunk + 64, slot, window)) {
    uint64_t fine_tail = kFineTail, fine_div = kFineDiv;
#if DSX_DIAG
    if (const char* v = getenv("DSX_FINE_TAIL")) fine_tail = (uint64_t)atol(v);
    if (const char* v = getenv("DSX_FINE_DIV")) fine_div = std::max<uint64_t>(1, atol(v));
#endif
    fine = std::max<uint64_t>(4096, (piece / fine_div) & ~4095ull);
    if (feeds && fine_tail && fine < piece) {
      const uint64_t last_ws = (nwin - 1) * W;
      fine_from = std::max(last_ws, (len - std::min(len, fine_tail)) / piece * piece);
    }
  }
};

// The GPU's shares of a one-window call during its read (run_index,
// run_ids): the points f_k = 1/2, 3/4, ... of the window where a digest on side
// stream k hashes the chunks completed since the previous point up to cut_k =
// the read time left after f_k over the GPU's ns per byte (its chain ends
// about when the read does; digest_pc_kernel beside the scans ran 37-40 ns
// per byte, profiles/r06an, so 45 with a margin: 0.892 against 0.872 x
// dsx_cut_fd at 58, profiles/r06ao).  They stop where cut_k falls below 1.5 x
// `feed_cut`, the host's usual cut (two points at 1 GiB and 12 threads; a
// third slowed the read, r06ab, r06am, r06ao); none when the first is below
// 2 x it.
struct Mid {
  uint64_t at, cut;
};
inline std::vector<Mid> plan_shares(uint64_t len, uint64_t max_chunk, uint64_t feed_cut) {
  double share_ns = kShareNsPerByte;  // the shares' chain, ns per byte
  double slack_ns = 0;              // a share may end this long after the read
  const double t_read = (double)len / kReadBytesPerNs;  // ns
  std::vector<double> fr;
  for (double f = 0.5; f < 0.99 && fr.size() < (size_t)kIdxSide; f = 0.5 * (1.0 + f)) fr.push_back(f);
#if DSX_DIAG
  if (const char* v = getenv("DSX_SHARE_NS")) share_ns = std::max(10.0, atof(v));
  if (const char* v = getenv("DSX_SHARE_SLACK")) slack_ns = 1e3 * atof(v);  // (us)
  if (const char* v = getenv("DSX_FEED_MID")) {  // (A/B: "0" off, else a list "0.5,0.75")
    fr.clear();
    for (const char* q = v; *q && fr.size() < (size_t)kIdxSide;) {
      char* nx = nullptr;
      const double f = strtod(q, &nx);
      if (nx == q) break;
      if (f > 0.05 && f < 0.99 && (fr.empty() || f > fr.back())) fr.push_back(f);
      q = *nx == ',' ? nx + 1 : nx;
    }
  }
#endif
  std::vector<Mid> mids;
  for (double f : fr) {
    const double ck = ((1.0 - f) * t_read + slack_ns) / share_ns;
    if (ck < (mids.empty() ? 2.0 : 1.5) * (double)feed_cut) break;
    mids.push_back({(uint64_t)(f * (double)len), std::min<uint64_t>(max_chunk, (uint64_t)ck & ~4095ull)});
  }
  return mids;
}

// The host's share of the tail: the feeder's SHA threads run beside the
// readers, within the process's CPU share; the GPU keeps the chunks up to
// feed_cut_for() bytes (a 58 ns/B chain at the end of the call), the host the
// longer ones.  Fewer threads hash less per ms, so the cut rises with them:
// 28 KiB at 28 threads (round 5's setting, above the share), 64 KiB at 12
// (tools/feed_ab.py).
constexpr uint64_t kFeedCutBase = 28ull << 10;  // at kFeedThreadsBase threads
constexpr int kFeedThreadsBase = 28;
inline uint64_t feed_cut_for(int64_t host_tail, int threads) {
  if (host_tail > 0) return (uint64_t)host_tail;  // forced (tests, A/B)
  const uint64_t cut = kFeedCutBase * (uint64_t)kFeedThreadsBase / (uint64_t)std::max(1, threads);
  return std::min<uint64_t>(128ull << 10, std::max<uint64_t>(kFeedCutBase, (cut + 2047) & ~4095ull));
}

// With the GPU's shares the host has fewer bytes: after the last point the
// feeder takes 11/16 of its usual cut (64 -> 44 KiB at 12 threads; 3/4:
// profiles/r06af, r06ag, 0.882 / 0.898 x dsx_cut_fd against 0.874 / 0.894 at
// 64; 44 against 48 / 40 / 36 KiB, r06aq: the call's end 1.88 ms after the
// last stitch against 2.04 / 1.89 / 2.07).
inline uint64_t share_end_cut(uint64_t fcut) {
  return std::max<uint64_t>(kFeedCutBase, (fcut * 11 / 16) & ~4095ull);
}

// run_index's schedule, decided before the read starts and executed by its
// read loop as it stands here: where a scan + stitch follows the pieces, which
// planned shares fire and where, and who hashes what in the last window.  The
// window's IDs come from three parties -- the GPU's shares, the feeder and the
// digest after the read -- that divide each segment's chunks by length at one
// cut: the GPU skips the chunks above it, the feeder takes exactly those.
// Both sides read that cut from the same ShareSeg, so no chunk is left
// between two cuts.
//   scan    the piece ends a scan + stitch follows: a window's end, every
//           scan_step bytes, every piece of the fine tail;
//   mids    the planned shares (plan_shares; `at` absolute); fire[k] is the
//           scan point share k fires at, 0: dropped.  A share fires at the
//           first scan point at or after its `at` that is below len and after
//           the previous share's (one per scan point: each has a snapshot and
//           a side stream of its own).  One that could fire only at len would
//           hash nothing during the read: it is dropped, and neither the
//           feeder nor the last digest ever sees its cut.  (Until round 7 the
//           feeder was built with the cuts of all planned shares and the last
//           digest with fcut_end: with a slot large enough that no scan point
//           below len followed a share's `at`, the last segment's chunks
//           between the two cuts were hashed by nobody.)
//   fired   the shares that fire, in order: {scan point, cut}; share j runs on
//           side stream side0 + j (side stream 0 carries the previous
//           window's digest when there is one);
//   segs    the last window's bytes [last_ws, len) cut at the fired shares'
//           scan points; a chunk belongs to the segment its end lies in
//           (from, to].  Segment j < fired.size() is share j's; the last one
//           is the digest's after the read, which starts from the last fired
//           share's snapshot (the window's start without one).  feed_cut
//           UINT64_MAX: no feeder; skip_above 0: the GPU hashes every chunk
//           (a share's cut of max or more).
struct ShareSeg {
  uint64_t from, to, feed_cut, skip_above;
};
struct IndexSchedule {
  bool feed_on = false;  // the last window has a tail feeder
  uint64_t last_ws = 0, fcut = 0, fcut_end = 0;
  size_t side0 = 0;
  std::vector<uint64_t> scan;
  std::vector<Mid> mids, fired;
  std::vector<uint64_t> fire;
  std::vector<ShareSeg> segs;
};
inline IndexSchedule index_schedule(const IndexGeom& g, uint64_t len, uint64_t max_chunk, int threads,
                                    int64_t host_tail, bool feeds) {
  IndexSchedule s;
  const PieceMap pm(len, g.piece, g.fine_from, g.fine);
  const uint64_t scan_step = std::max<uint64_t>(g.piece, kScanStep / g.piece * g.piece);
  for (uint64_t k = 0, scanned = 0; k < pm.np; ++k) {
    const uint64_t end = pm.off(k) + pm.size(k);
    const uint64_t wend = std::min(len, (end - 1) / g.W * g.W + g.W);  // its window's end
    if (end == wend || end - scanned >= scan_step || end > g.fine_from) {
      s.scan.push_back(end);
      scanned = end;
    }
  }
  s.last_ws = (g.nwin - 1) * g.W;
  s.side0 = g.nwin > 1 ? 1 : 0;
  s.fcut = s.fcut_end = feed_cut_for(host_tail, threads);
  s.feed_on = feeds;
  // (several windows: the last one's shares, on side streams 1..)
  bool share_multi = true;
#if DSX_DIAG
  if (g.nwin > 1 && getenv("DSX_FEED_MULTI") && atoi(getenv("DSX_FEED_MULTI")) == 0) s.feed_on = false;
  if (const char* v = getenv("DSX_SHARE_MULTI")) share_multi = atoi(v) != 0;
#endif
  if (s.feed_on && (g.nwin == 1 || share_multi) && host_tail < 0) {
    s.mids = plan_shares(len - s.last_ws, max_chunk, s.fcut);
    if (s.mids.size() > (size_t)kIdxSide - s.side0) s.mids.resize(kIdxSide - s.side0);
    for (Mid& m : s.mids) m.at += s.last_ws;
    s.fire.assign(s.mids.size(), 0);
    for (uint64_t sp : s.scan) {
      if (sp <= s.last_ws) continue;
      const size_t m = s.fired.size();
      if (sp >= len || m == s.mids.size()) break;
      if (sp >= s.mids[m].at) {
        s.fire[m] = sp;
        s.fired.push_back({sp, s.mids[m].cut});
      }
    }
    if (!s.fired.empty()) {
      s.fcut_end = share_end_cut(s.fcut);
#if DSX_DIAG
      if (const char* v = getenv("DSX_FEED_CUT_END")) s.fcut_end = std::max<uint64_t>(4096, atol(v));
#endif
    }
  }
  uint64_t from = s.last_ws;
  for (const Mid& m : s.fired) {
    s.segs.push_back({from, m.at, m.cut, m.cut >= max_chunk ? 0 : m.cut});
    from = m.at;
  }
  s.segs.push_back({from, len, s.feed_on ? s.fcut_end : UINT64_MAX, s.feed_on ? s.fcut_end : 0});
  return s;
}

// run_ids's schedule (VerifyIndex, ChopFile): the IDs of a given contiguous
// chunk list [start, ends[0]), [ends[0], ends[1]), ... (ends non-decreasing
// from start; the caller checked), decided before the read starts.  Offsets
// are relative to `start`: the call reads L = ends[n-1] - start bytes through
// windows that keep the list's longest chunk (maxc), so every chunk is hashed
// in the window where it ends.
//   win_i1  window w hashes the chunks [win_i1[w-1], win_i1[w]) (from 0):
//           those ending in (ws, ws + wl], window 0 also those ending at 0,
//           the last window the rest; i_last is the last window's first;
//   shares  the GPU's shares of the last window during its read (plan_shares
//           over its length, at most `sides`): share k takes the chunks that
//           end in the pieces landed by its point (`landed`, a multiple of
//           piece below L; chunks [previous i1, i1)) up to its cut;
//   early_cut  the host's usual cut at `threads` hashers (feed_cut_for);
//   end_cut    with shares, the last segment's: the lowest cut in 4 KiB steps
//           up to early_cut whose host bytes -- every segment's chunks above
//           its cut -- the threads finish at `host_ns` per byte within ~3/4
//           of the read (the list is known, so the host starts on the last
//           segment at once); early_cut where none fits, and without shares;
//   segs    the last window's chunks [i_last, n) by index.  Segment j <
//           shares.size() is share j's; the last one is the digest's after
//           the read.  The host hashes a segment's chunks longer than
//           feed_cut from the call's start (UINT64_MAX: the host tail is
//           off), the segment's digest skips those above skip_above (0: it
//           hashes every chunk -- a share's cut of maxc or more, or the tail
//           off).  run_ids reads both from here and computes no cut itself.
struct IdShare {
  uint64_t landed, cut, i1;
};
struct IdSeg {
  uint64_t i_from, i_to, feed_cut, skip_above;
};
struct IdsSchedule {
  WindowGeom g{};
  uint64_t L = 0, maxc = 0, last_ws = 0, i_last = 0;
  uint64_t early_cut = 0, end_cut = 0;
  std::vector<uint64_t> win_i1;
  std::vector<IdShare> shares;
  std::vector<IdSeg> segs;
};
inline IdsSchedule ids_schedule(uint64_t start, const uint64_t* ends, uint64_t n, uint64_t slot,
                                uint64_t window, int threads, int64_t host_tail, int sides, bool tail_on,
                                double host_ns) {
  IdsSchedule s;
  auto len_of = [&](uint64_t i) { return ends[i] - (i ? ends[i - 1] : start); };
  for (uint64_t i = 0; i < n; ++i) s.maxc = std::max(s.maxc, len_of(i));
  s.L = n ? ends[n - 1] - start : 0;
  const uint64_t L = s.L;
  s.g = window_geom(L, s.maxc, slot, window);
  const uint64_t piece = s.g.piece, W = s.g.W, nwin = s.g.nwin;
  s.win_i1.assign(nwin, n);
  for (uint64_t w = 0, i = 0; w + 1 < nwin; ++w) {
    while (i < n && ends[i] - start <= (w + 1) * W) ++i;
    s.win_i1[w] = i;
  }
  s.last_ws = (nwin - 1) * W;
  s.i_last = nwin > 1 ? s.win_i1[nwin - 2] : 0;
  s.early_cut = s.end_cut = feed_cut_for(host_tail, threads);
  // (several windows: the last one's shares, planned over its length)
  bool share_multi = true;
#if DSX_DIAG
  if (const char* v = getenv("DSX_SHARE_MULTI")) share_multi = atoi(v) != 0;
#endif
  if (tail_on && (nwin == 1 || share_multi) && host_tail < 0) {
    for (const Mid& m : plan_shares(L - s.last_ws, s.maxc, s.early_cut)) {
      const uint64_t landed = std::min(L, (s.last_ws + m.at + piece - 1) / piece * piece);
      if (landed >= L || s.shares.size() >= (size_t)std::max(0, sides)) break;
      uint64_t i1 = s.shares.empty() ? s.i_last : s.shares.back().i1;
      while (i1 < n && ends[i1] - start <= landed) ++i1;
      s.shares.push_back({landed, m.cut, i1});
    }
    if (!s.shares.empty()) {
      // host bytes: each segment's chunks above its cut, and the last
      // segment's above end_cut
      uint64_t fixed = 0;
      std::vector<uint64_t> last;
      for (uint64_t i = s.i_last, k = 0; i < n; ++i) {
        while (k < s.shares.size() && i >= s.shares[k].i1) ++k;
        const uint64_t ln = len_of(i);
        if (k < s.shares.size()) {
          if (ln > s.shares[k].cut) fixed += ln;
        } else {
          last.push_back(ln);
        }
      }
      std::sort(last.begin(), last.end());
      const double budget = 0.75 * (double)L / kReadBytesPerNs * threads / host_ns;  // bytes
      // the lowest cut (4 KiB steps up to early_cut) whose host bytes fit
      uint64_t tail_bytes = 0;
      for (uint64_t x : last) tail_bytes += x;
      size_t j = 0;
      for (uint64_t cut = 4096; cut <= s.early_cut; cut += 4096) {
        while (j < last.size() && last[j] <= cut) tail_bytes -= last[j++];
        if ((double)(fixed + tail_bytes) <= budget) {
          s.end_cut = cut;
          break;
        }
      }
#if DSX_DIAG
      if (const char* v = getenv("DSX_FEED_CUT_END")) s.end_cut = std::max<uint64_t>(4096, atol(v));
#endif
    }
  }
  uint64_t from = s.i_last;
  for (const IdShare& sh : s.shares) {
    s.segs.push_back({from, sh.i1, sh.cut, sh.cut >= s.maxc ? 0 : sh.cut});
    from = sh.i1;
  }
  const uint64_t cut = s.shares.empty() ? s.early_cut : s.end_cut;
  s.segs.push_back({from, n, tail_on ? cut : UINT64_MAX, tail_on ? cut : 0});
  return s;
}

}  // namespace dsx_host
#endif  // DSX_INDEX_PLAN_H_
