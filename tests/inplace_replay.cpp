// inplace_replay.cpp -- dsx_inplace_plan.h under a host sanitizer, without Python:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude tests/inplace_replay.cpp -o inplace_replay
//   ./inplace_replay
// A seeded sweep of old / new versions over small alphabets of blocks and the
// crafted arrays of tests/test_inplace_host.py go through
// dsx_host::inplace_plan, and every schedule through a brute-force executor
// of this file's own: bytes are identities (old byte x is the number x), each
// launch reads everything before it writes anything, and a read of a byte an
// earlier launch wrote, a write outside the launch's window, a read inside
// it, a stash byte that is not what the target wants, or a final buffer that
// is not the target is a failure.  Prints "<cases> cases, <n> failures".
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../desync_amd/csrc/dsx_inplace_plan.h"

namespace {

typedef uint64_t u64;
typedef int64_t i64;
constexpr i64 kZero = -1, kGarbage = -2, kStoreBase = 1ll << 40;

struct Rng {
  u64 s;
  u64 next() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return s;
  }
  u64 below(u64 n) { return next() % n; }
  bool chance(int pct) { return below(100) < (u64)pct; }
};

struct Case {
  std::vector<dsx_plan_seg_t> segs;
  std::vector<u64> ends;
  std::vector<uint8_t> keep;
  bool has_keep = false;
  u64 have_len = 0, new_len = 0;
};

dsx_plan_seg_t mk(u64 dst, u64 bytes, u64 src_off, uint32_t first, uint32_t count, int32_t source) {
  dsx_plan_seg_t g{};
  g.dst_off = dst, g.bytes = bytes, g.src_off = src_off, g.first = first, g.count = count;
  g.source = source, g.seed_first = 0xFFFFFFFFu;
  return g;
}

i64 ident(int32_t source, u64 off) {
  if (source == DSX_SRC_NULL) return kZero;
  if (source == DSX_SRC_SELF) return (i64)off;
  return (source == DSX_SRC_STORE ? kStoreBase : (source + 2) * kStoreBase) + (i64)off;
}

int fails = 0;
void fail(const char* what, u64 id) {
  if (++fails <= 20) fprintf(stderr, "case %llu: %s\n", (unsigned long long)id, what);
}

// runs the schedule; true when every check held
bool execute(const Case& c, const dsx_host::InplacePlan& p, u64 skew, u64 window, u64 id) {
  const u64 cap = std::max(c.have_len, c.new_len);
  std::vector<i64> buf(cap), want(cap), stash(p.totals.stash_peak, kGarbage);
  std::vector<uint8_t> written(cap, 0), may(cap, 0), saved(p.totals.stash_peak, 0);
  for (u64 x = 0; x < cap; ++x) buf[x] = want[x] = x < c.have_len ? (i64)x : kGarbage;
  for (const dsx_plan_seg_t& g : c.segs) {
    const bool same = g.source == DSX_SRC_SELF && g.src_off == g.dst_off;
    for (u64 k = g.first; k < (u64)g.first + g.count; ++k) {
      if (same || (c.has_keep && c.keep[k])) continue;
      for (u64 x = k ? c.ends[k - 1] : 0; x < c.ends[k]; ++x) {
        want[x] = ident(g.source, g.src_off + (x - g.dst_off));
        may[x] = 1;
      }
    }
  }
  bool ok = true;
  auto bad = [&](const char* what) {
    if (ok) fail(what, id);
    ok = false;
  };
  u64 nwrite = 0, nsave = 0;
  std::vector<i64> vals;
  for (const dsx_inplace_launch_t& l : p.launches) {
    if (l.seg0 + l.nsegs > p.segs.size() || !l.nsegs) return bad("a launch's table is out of range"), false;
    const u64 w0 = l.window * window > skew ? l.window * window - skew : 0;
    const u64 w1 = (l.window + 1) * window - skew;
    const bool save = l.kind == DSX_INPLACE_SAVE;
    vals.clear();
    u64 prev = 0;
    for (u64 j = l.seg0; j < l.seg0 + l.nsegs; ++j) {  // every read first
      const dsx_plan_seg_t& g = p.segs[j];
      if (!g.bytes || g.dst_off < prev || g.dst_off < l.lo || g.dst_off + g.bytes > l.hi)
        return bad("a table does not ascend inside [lo, hi)"), false;
      prev = g.dst_off + g.bytes;
      if (save) {
        if (g.source != DSX_SRC_SELF || g.src_off < w0 || g.src_off + g.bytes > std::min(w1, c.have_len))
          return bad("SAVE reads outside its window"), false;
        if (g.dst_off + g.bytes > stash.size()) return bad("SAVE writes beyond the peak"), false;
      } else {
        if (g.dst_off < w0 || g.dst_off + g.bytes > std::min(w1, c.new_len))
          return bad("WRITE writes outside its window"), false;
        if (g.source == DSX_SRC_SELF &&
            (g.src_off + g.bytes > c.have_len ||
             !(g.src_off + g.bytes <= w0 || g.src_off >= std::min(w1, c.new_len))))
          return bad("WRITE reads the buffer inside its window"), false;
        if (g.source == DSX_SRC_STASH && g.src_off + g.bytes > stash.size())
          return bad("WRITE reads beyond the stash"), false;
        if (g.source < DSX_SRC_STASH) return bad("an unknown source"), false;
      }
      for (u64 b = 0; b < g.bytes; ++b) {
        if (g.source == DSX_SRC_SELF) {
          if (written[g.src_off + b]) bad("a read of a byte an earlier launch wrote");
          vals.push_back(buf[g.src_off + b]);
        } else if (g.source == DSX_SRC_STASH) {
          if (!saved[g.src_off + b]) bad("a stash byte read before it was saved");
          if (stash[g.src_off + b] != want[g.dst_off + b]) bad("the stash holds another byte");
          vals.push_back(stash[g.src_off + b]);
        } else {
          vals.push_back(ident(g.source, g.src_off + b));
        }
      }
    }
    u64 v = 0;
    for (u64 j = l.seg0; j < l.seg0 + l.nsegs; ++j) {  // then every write
      const dsx_plan_seg_t& g = p.segs[j];
      for (u64 b = 0; b < g.bytes; ++b, ++v) {
        if (save) {
          stash[g.dst_off + b] = vals[v], saved[g.dst_off + b] = 1, ++nsave;
        } else {
          if (written[g.dst_off + b]) bad("a byte is written twice");
          if (!may[g.dst_off + b]) bad("a byte nobody was to write is written");
          buf[g.dst_off + b] = vals[v], written[g.dst_off + b] = 1, ++nwrite;
        }
      }
    }
  }
  for (u64 x = 0; x < cap; ++x) {
    if (x < c.new_len && buf[x] != want[x]) bad("the buffer is not the target");
    if (x >= c.new_len && written[x]) bad("a byte beyond new_len is written");
    if (may[x] != written[x]) bad("a byte of the target was left out");
  }
  if (nwrite != p.totals.written_bytes || nsave != p.totals.stash_bytes) bad("the totals are off");
  if (p.totals.stash_peak > c.have_len) bad("the peak exceeds have_len");
  return ok;
}

// plans and executes one case in the three direction modes
void run_case(const Case& c, u64 skew, u64 tile, u64 window, u64 id) {
  u64 peak[3] = {0, 0, 0};
  const uint32_t modes[3] = {0, DSX_INPLACE_ASCENDING, DSX_INPLACE_DESCENDING};
  for (int m = 0; m < 3; ++m) {
    dsx_host::InplacePlan p;
    const int rc = dsx_host::inplace_plan(c.segs.data(), c.segs.size(), c.ends.data(), c.ends.size(),
                                          c.has_keep ? c.keep.data() : nullptr, c.have_len, c.new_len,
                                          skew, tile, window, c.have_len, modes[m], &p);
    if (rc != DSX_OK) {  // stash_cap = have_len: no case may be refused
      fail("refused", id);
      return;
    }
    peak[m] = p.totals.stash_peak;
    if (!execute(c, p, skew, window, id)) return;
  }
  if (peak[0] != std::min(peak[1], peak[2])) fail("the free choice is not the smaller peak", id);
}

Case random_case(Rng& r) {
  Case c;
  const u64 k = 1 + r.below(4);
  static const u64 kSizes[8] = {1, 3, 7, 15, 16, 17, 33, 70};
  u64 size[7];
  for (u64 s = 0; s < k + 3; ++s) size[s] = kSizes[r.below(8)];
  std::vector<u64> old_sym(r.below(13)), new_sym(r.below(13));
  for (u64& s : old_sym) s = r.below(k);
  for (u64& s : new_sym) s = r.chance(25) ? r.below(k + 3) : r.below(k);
  if (r.chance(30) && !old_sym.empty()) {  // a shifted copy
    const u64 cut = r.below(old_sym.size() + 1);
    new_sym.assign(old_sym.begin() + cut, old_sym.end());
    if (r.chance(50)) new_sym.insert(new_sym.end(), old_sym.begin(), old_sym.begin() + cut);
    if (r.chance(30)) new_sym.insert(new_sym.begin(), r.below(k + 3));
  }
  std::vector<std::vector<u64>> where(k + 3);
  u64 at = 0;
  for (u64 s : old_sym) where[s].push_back(at), at += size[s];
  c.have_len = at;
  c.has_keep = r.chance(70);
  u64 ext[4] = {0, 0, 0, 0};
  at = 0;
  for (u64 i = 0; i < new_sym.size(); ++i) {
    const u64 s = new_sym[i], n = size[s];
    bool in_place = false;
    for (u64 o : where[s]) in_place |= o == at;
    const bool kp = in_place && r.chance(50);
    c.keep.push_back(kp);
    int32_t src;
    u64 off;
    if (!where[s].empty() && !(kp && r.chance(50))) {
      src = DSX_SRC_SELF;
      off = in_place && r.chance(70) ? at : where[s][r.below(where[s].size())];
    } else {
      static const int32_t kExt[4] = {DSX_SRC_NULL, DSX_SRC_STORE, 0, 1};
      const u64 e = s >= k ? s % 4 : 1;
      src = kExt[e];
      off = src == DSX_SRC_NULL ? 0 : ext[e];
      ext[e] += n;
    }
    if (!c.segs.empty() && c.segs.back().source == src && r.chance(80) &&
        (src == DSX_SRC_NULL || c.segs.back().src_off + c.segs.back().bytes == off)) {
      c.segs.back().bytes += n, c.segs.back().count += 1;
    } else {
      c.segs.push_back(mk(at, n, off, (uint32_t)i, 1, src));
    }
    at += n;
    c.ends.push_back(at);
  }
  c.new_len = at;
  if (!c.has_keep) c.keep.clear();
  if (r.chance(10) && !c.segs.empty()) c.segs.erase(c.segs.begin() + r.below(c.segs.size()));
  return c;
}

std::vector<u64> chunks(u64 total, u64 size) {
  std::vector<u64> e;
  for (u64 x = size; x < total; x += size) e.push_back(x);
  e.push_back(total);
  return e;
}

int expect_rc(const Case& c, u64 skew, u64 tile, u64 window, u64 cap, uint32_t flags, int want,
              u64 id) {
  dsx_host::InplacePlan p;
  const int rc = dsx_host::inplace_plan(c.segs.data(), c.segs.size(), c.ends.data(), c.ends.size(),
                                        c.has_keep ? c.keep.data() : nullptr, c.have_len, c.new_len,
                                        skew, tile, window, cap, flags, &p);
  if (rc != want) fail("an unexpected return code", id);
  if (rc != DSX_OK && (!p.launches.empty() || !p.segs.empty())) fail("a refusal lists launches", id);
  return rc;
}

}  // namespace

int main() {
  u64 cases = 0;
  Rng r{0x9E3779B97F4A7C15ull};
  const u64 tile = 16;
  for (int i = 0; i < 4000; ++i, ++cases) {
    const Case c = random_case(r);
    static const u64 kSkew[4] = {0, 0, 1, 15};
    run_case(c, kSkew[r.below(4)], tile, r.chance(50) ? 16 : 64, cases);
  }
  // ---- crafted: shifts, swapped halves, a straddling source, five windows ----
  for (u64 window : {(u64)16, (u64)64})
    for (u64 delta : {(u64)1, tile - 1, window, 3 * window + 5}) {
      const u64 body = 10 * window;
      Case del;  // the old version without its first delta bytes
      del.ends = chunks(body, 24);
      del.segs = {mk(0, body, delta, 0, (uint32_t)del.ends.size(), DSX_SRC_SELF)};
      del.have_len = body + delta, del.new_len = body;
      run_case(del, 0, tile, window, cases++);
      Case ins;  // delta store bytes, then the old version
      ins.ends = chunks(body, 24);
      for (u64& e : ins.ends) e += delta;
      ins.ends.insert(ins.ends.begin(), delta);
      ins.segs = {mk(0, delta, 0, 0, 1, DSX_SRC_STORE),
                  mk(delta, body, 0, 1, (uint32_t)ins.ends.size() - 1, DSX_SRC_SELF)};
      ins.have_len = body, ins.new_len = body + delta;
      run_case(ins, 0, tile, window, cases++);
      for (const Case* c : {&del, &ins}) {
        dsx_host::InplacePlan p;
        dsx_host::inplace_plan(c->segs.data(), c->segs.size(), c->ends.data(), c->ends.size(), nullptr,
                               c->have_len, c->new_len, 0, tile, window, c->have_len, 0, &p);
        const u64 wantp = delta >= window ? 0 : window - delta;
        if (p.totals.stash_peak != wantp) fail("a shift's peak", cases);
        if (p.totals.direction != (c == &del ? DSX_INPLACE_ASCENDING : DSX_INPLACE_DESCENDING))
          fail("a shift's direction", cases);
      }
    }
  {
    Case sw;
    const u64 half = 160;
    sw.ends = chunks(2 * half, 20);
    sw.segs = {mk(0, half, half, 0, 8, DSX_SRC_SELF), mk(half, half, 0, 8, 8, DSX_SRC_SELF)};
    sw.have_len = sw.new_len = 2 * half;
    run_case(sw, 0, tile, 64, cases++);
    expect_rc(sw, 0, tile, 64, half, 0, DSX_OK, cases);
    expect_rc(sw, 0, tile, 64, half - 1, 0, DSX_E_CAPACITY, cases++);
    Case st;
    st.ends = {64, 96, 128};
    st.segs = {mk(64, 32, 50, 1, 1, DSX_SRC_SELF)};
    st.have_len = st.new_len = 128;
    run_case(st, 0, tile, 64, cases++);
    Case five;
    five.ends = chunks(5 * 64 + 40, 90);
    five.segs = {mk(0, five.ends.back(), 7, 0, (uint32_t)five.ends.size(), DSX_SRC_SELF)};
    five.have_len = five.ends.back() + 7, five.new_len = five.ends.back();
    run_case(five, 3, tile, 64, cases++);
    Case idt;
    idt.ends = chunks(300, 20);
    idt.segs = {mk(0, 300, 0, 0, 15, DSX_SRC_SELF)};
    idt.have_len = idt.new_len = 300;
    dsx_host::InplacePlan p;
    if (dsx_host::inplace_plan(idt.segs.data(), 1, idt.ends.data(), 15, nullptr, 300, 300, 0, tile, 64,
                               0, 0, &p) != DSX_OK || !p.launches.empty() || p.totals.kept_chunks != 15)
      fail("identity", cases);
    ++cases;
  }
  // ---- crafted arrays: every refusal, nothing may index out of bounds ----------
  {
    Case g;
    g.ends = {40, 100};
    g.have_len = g.new_len = 100;
    auto with = [&](std::vector<dsx_plan_seg_t> segs) {
      Case c = g;
      c.segs = std::move(segs);
      return c;
    };
    const dsx_plan_seg_t a = mk(0, 40, 60, 0, 1, DSX_SRC_SELF), b = mk(40, 60, 0, 1, 1, DSX_SRC_STORE);
    const u64 big = 1ull << 20;
    expect_rc(with({a, b}), 0, tile, 16, big, 0, DSX_OK, cases++);
    expect_rc(with({b, a}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({a, mk(30, 70, 0, 1, 1, DSX_SRC_STORE)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({mk(0, 40, 61, 0, 1, DSX_SRC_SELF)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({mk(0, 40, UINT64_MAX - 7, 0, 1, DSX_SRC_SELF)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({mk(40, 60, 0, 1, 2, DSX_SRC_STORE)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({mk(40, 60, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, DSX_SRC_STORE)}), 0, tile, 16, big, 0,
              DSX_E_INVAL, cases++);
    expect_rc(with({mk(40, 60, 0, 2, 0, DSX_SRC_STORE)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({mk(0, 41, 0, 0, 1, DSX_SRC_STORE)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({mk(1, 40, 0, 0, 1, DSX_SRC_STORE)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({mk(0, 40, 0, 0, 1, -5)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({mk(0, UINT64_MAX, 0, 0, 1, DSX_SRC_STORE)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({mk(UINT64_MAX - 3, 40, 0, 0, 1, DSX_SRC_STORE)}), 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    Case dec = with({a, b});
    dec.ends = {100, 40};
    expect_rc(dec, 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    dec.ends = {40, 101};
    expect_rc(dec, 0, tile, 16, big, 0, DSX_E_INVAL, cases++);
    for (u64 w : {(u64)0, (u64)8, (u64)24}) expect_rc(with({a, b}), 0, tile, w, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({a, b}), 0, 0, 16, big, 0, DSX_E_INVAL, cases++);
    expect_rc(with({a, b}), tile, tile, 16, big, 0, DSX_E_INVAL, cases++);
    for (uint32_t f : {1u, 128u, 256u, DSX_INPLACE_ASCENDING | DSX_INPLACE_DESCENDING, 1u << 31})
      expect_rc(with({a, b}), 0, tile, 16, big, f, DSX_E_INVAL, cases++);
    expect_rc(with({a, b}), 0, tile, 16, 39, DSX_INPLACE_DESCENDING, DSX_E_CAPACITY, cases++);
    Case kp = with({a, b});  // a keep mask as long as the chunks, one set
    kp.has_keep = true, kp.keep = {0, 1};
    run_case(kp, 0, tile, 16, cases++);
  }
  printf("inplace_replay: %llu cases, %d failures\n", (unsigned long long)cases, fails);
  return fails ? 1 : 0;
}
