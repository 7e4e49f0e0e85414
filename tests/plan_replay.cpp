// plan_replay.cpp -- dsx_plan_walk under a host sanitizer, without Python:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -Iinclude tests/plan_replay.cpp desync_amd/csrc/dsx_plan.cpp -o plan_replay
//   ./plan_replay
//
// Replays, against a brute-force sequencer written here (every occurrence,
// chunk by chunk: sequencer.go:56-74, fileseed.go:42-80, :114-136,
// nullseed.go:45-74), the random ID strings of tests/test_plan_host.py at
// limits 0, 1, 2, 3, 5 and 100, the ABAB... input at 2,000 chunks, and the
// crafted arrays, which must each return DSX_E_INVAL.  Exit status 0: all
// agreed.  dsx_plan.cpp includes nothing of HIP, so no GPU runtime is linked.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "dsx.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
uint64_t rng_state = 0x243F6A8885A308D3ull;
uint32_t rnd(uint32_t n) {  // [0, n)
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((rng_state >> 33) % n);
}

struct Seed {
  std::vector<int> ids;
  std::vector<uint64_t> sizes;
};
struct Case {
  std::vector<int> ids;
  std::vector<uint64_t> sizes;
  std::vector<Seed> seeds;
  int null_id = -1;  // -1: no null seed
  uint64_t start = 0;
};

std::vector<uint64_t> ends_of(const std::vector<uint64_t>& sizes, uint64_t start) {
  std::vector<uint64_t> e(sizes.size());
  uint64_t at = start;
  for (size_t i = 0; i < sizes.size(); ++i) e[i] = at += sizes[i];
  return e;
}

struct Out {
  std::vector<dsx_plan_seg_t> segs;
  std::vector<uint32_t> store;
  dsx_plan_totals_t tot{};
};

Out brute(const Case& c, uint32_t limit) {
  Out o;
  const size_t n = c.ids.size();
  const std::vector<uint64_t> ends = ends_of(c.sizes, c.start);
  std::vector<std::vector<uint64_t>> sends;
  for (const Seed& s : c.seeds) sends.push_back(ends_of(s.sizes, 0));
  std::map<int, uint64_t> store_off;
  for (size_t cur = 0; cur < n;) {
    uint64_t max = 0, advance = 1;
    int32_t source = DSX_SRC_STORE;
    uint32_t first = kNone;
    auto tstart = [&](size_t i) { return i ? ends[i - 1] : c.start; };
    if (c.null_id >= 0) {
      uint64_t k = 0;
      while (cur + k < n && !(limit && k == limit) && c.ids[cur + k] == c.null_id) ++k;
      if (k && ends[cur + k - 1] - tstart(cur) > max) source = DSX_SRC_NULL, advance = k, max = ends[cur + k - 1] - tstart(cur);
    }
    for (size_t si = 0; si < c.seeds.size(); ++si) {
      const Seed& s = c.seeds[si];
      uint64_t best = 0;
      size_t bp = 0;
      for (size_t p = 0; p < s.ids.size(); ++p) {
        if (s.ids[p] != c.ids[cur]) continue;
        uint64_t k = 0;
        while (!(limit && k == limit) && p + k < s.ids.size() && cur + k < n && c.ids[cur + k] == s.ids[p + k]) ++k;
        if (k > best) best = k, bp = p;
        if (limit && best == limit) break;
      }
      if (!best) continue;
      const uint64_t size = sends[si][bp + best - 1] - (bp ? sends[si][bp - 1] : 0);
      if (size > max) source = (int32_t)si, first = (uint32_t)bp, advance = best, max = size;
    }
    dsx_plan_seg_t g{};
    g.dst_off = tstart(cur);
    g.bytes = ends[cur + advance - 1] - g.dst_off;
    g.first = (uint32_t)cur, g.count = (uint32_t)advance, g.source = source, g.seed_first = first;
    if (source >= 0) {
      g.src_off = first ? sends[source][first - 1] : 0;
      o.tot.seed_chunks += advance, o.tot.seed_bytes += g.bytes;
    } else if (source == DSX_SRC_NULL) {
      o.tot.null_chunks += advance, o.tot.null_bytes += g.bytes;
    } else {
      auto it = store_off.find(c.ids[cur]);
      if (it == store_off.end()) {
        it = store_off.emplace(c.ids[cur], o.tot.store_len).first;
        o.store.push_back((uint32_t)cur);
        o.tot.store_len += g.bytes;
      }
      g.src_off = it->second;
      o.tot.store_chunks += 1, o.tot.store_bytes += g.bytes;
    }
    o.segs.push_back(g);
    cur += advance;
  }
  o.tot.segments = o.segs.size();
  o.tot.store_unique = o.store.size();
  return o;
}

struct Classes {
  std::vector<uint64_t> ends;
  std::vector<uint32_t> first_pos;
  std::vector<uint8_t> is_null;
  std::vector<std::vector<uint32_t>> tclass, sclass;
  std::vector<std::vector<uint64_t>> sends;
  std::vector<dsx_plan_seed_t> ps;
};

Classes classes_of(const Case& c) {
  Classes k;
  const size_t n = c.ids.size();
  k.ends = ends_of(c.sizes, c.start);
  std::map<int, uint32_t> seen;
  for (size_t i = 0; i < n; ++i) k.first_pos.push_back(seen.emplace(c.ids[i], (uint32_t)i).first->second);
  for (size_t i = 0; i < n; ++i) k.is_null.push_back(c.ids[i] == c.null_id);
  for (const Seed& s : c.seeds) {
    std::map<int, uint32_t> low;
    std::vector<uint32_t> sc, tc;
    for (size_t p = 0; p < s.ids.size(); ++p) sc.push_back(low.emplace(s.ids[p], (uint32_t)p).first->second);
    for (size_t i = 0; i < n; ++i) tc.push_back(low.count(c.ids[i]) ? low[c.ids[i]] : kNone);
    k.sclass.push_back(sc), k.tclass.push_back(tc), k.sends.push_back(ends_of(s.sizes, 0));
  }
  for (size_t s = 0; s < c.seeds.size(); ++s)
    k.ps.push_back(dsx_plan_seed_t{k.tclass[s].data(), k.sclass[s].data(), k.sends[s].data(), c.seeds[s].ids.size()});
  return k;
}

int walk(const Case& c, const Classes& k, uint32_t limit, Out* o) {
  const size_t n = c.ids.size();
  o->segs.assign(n + 1, dsx_plan_seg_t{});
  o->store.assign(n + 1, 0);
  const int rc = dsx_plan_walk(k.ends.data(), c.start, n, k.first_pos.data(), c.null_id >= 0 ? k.is_null.data() : nullptr,
                               k.ps.data(), (uint32_t)k.ps.size(), limit, o->segs.data(), n, o->store.data(), n, &o->tot);
  if (rc == DSX_OK) o->segs.resize(o->tot.segments), o->store.resize(o->tot.store_unique);
  return rc;
}

bool same(const Out& a, const Out& b) {
  if (a.segs.size() != b.segs.size() || a.store != b.store) return false;
  for (size_t i = 0; i < a.segs.size(); ++i) {
    const dsx_plan_seg_t &x = a.segs[i], &y = b.segs[i];
    if (x.dst_off != y.dst_off || x.bytes != y.bytes || x.src_off != y.src_off || x.first != y.first ||
        x.count != y.count || x.source != y.source || x.seed_first != y.seed_first)
      return false;
  }
  const dsx_plan_totals_t &s = a.tot, &t = b.tot;
  return s.segments == t.segments && s.seed_chunks == t.seed_chunks && s.seed_bytes == t.seed_bytes &&
         s.null_chunks == t.null_chunks && s.null_bytes == t.null_bytes && s.store_chunks == t.store_chunks &&
         s.store_bytes == t.store_bytes && s.store_unique == t.store_unique && s.store_len == t.store_len;
}

Case random_case() {
  Case c;
  const int k = 1 + rnd(4);
  const size_t n = 1 + rnd(60);
  for (size_t i = 0; i < n; ++i) c.ids.push_back(rnd(k)), c.sizes.push_back(1 + rnd(4));
  const int nseeds = 1 + rnd(3);
  for (int s = 0; s < nseeds; ++s) {
    Seed sd;
    const size_t m = 1 + rnd(60);
    if (rnd(10) < 4) {  // a stretch of the target behind a short random prefix
      for (uint32_t j = rnd(6); j > 0; --j) sd.ids.push_back(rnd(k));
      for (size_t a = rnd((uint32_t)n); a < n && sd.ids.size() < m; ++a) sd.ids.push_back(c.ids[a]);
    }
    while (sd.ids.size() < m && (sd.ids.empty() || rnd(10) < 9)) sd.ids.push_back(rnd(k));
    for (size_t p = 0; p < sd.ids.size(); ++p) sd.sizes.push_back(1 + rnd(4));
    c.seeds.push_back(sd);
  }
  const uint32_t pick = rnd(4);
  c.null_id = pick == 0 ? -1 : pick == 3 ? k : 0;
  c.start = rnd(3) == 0 ? 7 : 0;
  return c;
}

int fails = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s\n", what);
    ++fails;
  }
}

}  // namespace

int main() {
  const uint32_t limits[] = {0, 1, 2, 3, 5, 100};
  // case 2: random ID strings
  uint64_t cases = 0;
  for (uint32_t limit : limits)
    for (int r = 0; r < 2000; ++r) {
      const Case c = random_case();
      const Classes k = classes_of(c);
      Out got;
      const int rc = walk(c, k, limit, &got);
      expect(rc == DSX_OK && same(got, brute(c, limit)), "random ID string");
      ++cases;
    }
  // case 4: ABAB...
  for (uint32_t limit : {0u, 100u}) {
    Case c;
    for (int i = 0; i < 2000; ++i) c.ids.push_back(i & 1), c.sizes.push_back(1 + i % 3);
    Seed a, b;
    for (int i = 0; i < 1997; ++i) a.ids.push_back((i + 1) & 1), a.sizes.push_back(2);
    for (int i = 0; i < 700; ++i) b.ids.push_back(i & 1), b.sizes.push_back(3);
    c.seeds = {a, b};
    const Classes k = classes_of(c);
    Out got;
    expect(walk(c, k, limit, &got) == DSX_OK && same(got, brute(c, limit)), "ABAB");
    ++cases;
  }
  // case 5: crafted arrays (target ABCA, seed BCAB, then one word spoiled)
  {
    Case c;
    c.ids = {0, 1, 2, 0}, c.sizes = {5, 6, 7, 5};
    c.seeds = {Seed{{1, 2, 0, 1}, {6, 7, 5, 6}}};
    for (int what = 0; what <= 9; ++what) {
      Classes k = classes_of(c);
      Case cc = c;
      switch (what) {
        case 0: break;                                    // well formed
        case 1: k.sclass[0][1] = 3; break;                // sclass[p] > p
        case 2: k.sclass[0] = {0, 0, 1, 0}; break;        // not a fixed point
        case 3: k.tclass[0][2] = 4; break;                // == m
        case 4: k.tclass[0][0] = 0xFFFFFFFEu; break;
        case 5: k.tclass[0][0] = 3; break;                // sclass[3] == 0
        case 6: k.first_pos[1] = 2; break;                // above i
        case 7: k.ends[2] = k.ends[1] - 1; break;
        case 8: k.sends[0][3] = 1; break;
        case 9: cc.start = 6; break;                      // ends[0] below start
      }
      Out got;
      const int rc = walk(cc, k, 0, &got);
      expect(rc == (what == 0 ? DSX_OK : DSX_E_INVAL), "crafted arrays");
      ++cases;
    }
    dsx_plan_totals_t t;
    expect(dsx_plan_walk(nullptr, 0, 0xFFFFFFF1ull, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, 0, &t) ==
               DSX_E_INVAL, "n above the limit");
    dsx_plan_seed_t big{nullptr, nullptr, nullptr, 0xFFFFFFF1ull};
    expect(dsx_plan_walk(nullptr, 0, 0, nullptr, nullptr, &big, 1, 0, nullptr, 0, nullptr, 0, &t) == DSX_E_INVAL,
           "m above the limit");
    // capacity: the counts come back, nothing is written past the caps
    Classes k = classes_of(c);
    Out got;
    got.segs.assign(1, dsx_plan_seg_t{});
    const int rc = dsx_plan_walk(k.ends.data(), 0, 4, k.first_pos.data(), nullptr, k.ps.data(), 1, 1, got.segs.data(), 1,
                                 nullptr, 0, &got.tot);
    expect(rc == DSX_E_CAPACITY && got.tot.segments == 4, "capacity");
  }
  printf("plan_replay: %llu cases, %d failures\n", (unsigned long long)cases, fails);
  return fails ? 1 : 0;
}
