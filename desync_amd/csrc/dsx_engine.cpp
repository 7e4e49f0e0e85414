// dsx_engine.cpp -- host engine of libdsx.so (declared in dsx_engine.h).
//
// The engine splits a blob into pieces, and per piece enqueues on the
// context's HIP stream: scan (dsx_scan.hip) -> walk -> fixup -> gather
// (dsx_stitch.hip).  The chain position is carried between pieces in device
// memory (DevState.carry), so a multi-piece call needs no host round trip
// until the end.  The C ABI over it is dsx_api.cpp (cut lists, shards),
// dsx_index.cpp and dsx_stream.cpp; a piece's scan geometry is
// dsx_scan_geom.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>

#include "dsx_engine.h"

using namespace dsx;

TestConsts make_tc(const dsx_params_t* p) {
  TestConsts tc;
  tc.d = p->discriminator;
  tc.dm1 = p->discriminator - 1u;
  tc.inv = p->inverse_odd;
  tc.qmax = p->qmax;
  tc.qbias = p->qbias;
  tc.rot = (uint32_t)p->rot;
  tc.rcp = 1.0f / (float)p->discriminator;
  // MODE 1 (is_cand in dsx_scan.hip): fma(h, 1/d, 1.5*2^23 - 1) puts
  // round(h/d) - 1 + 0x400000 in the low mantissa bits; madc folds the
  // 0x400000*d offset and the -1 back into the exact 24-bit check.
  tc.c0 = 12582911.0f;
  tc.madc = p->discriminator - 1u - (p->discriminator << 22);
  // MODE 2 prefilter: with d = 2^k * dodd, h + 1 = d*m (1 <= m <= 2^32/d)
  // gives t = (h+1)*inv - 1 = 2^k*m - 1 < 2^k*floor(2^32/d) = vmax (exact
  // for odd d; for even d the rare path re-checks h % d == d-1)
  const uint32_t k = (uint32_t)p->rot;
  tc.tadd = p->inverse_odd - 1u;
  tc.vmax = (uint32_t)(((1ull << 32) / p->discriminator) << k);
  tc.dodd = p->discriminator >> k;
  // scanl keeps ~h in the hash register (the same recurrence from ~0), so
  // t + 1 = (h+1)*inv = (~h)*(2^32 - inv) is one v_mul_lo_u32
  tc.ninv = 0u - p->inverse_odd;
  tc.vmax1 = tc.vmax + 1u;
  return tc;
}

// MODE 2 (multiply-inverse prefilter, DESIGN.md "Boundary test") for every d
// that is not a power of two; MODE 1 (float, exact for 1024 < d < 2^22) or
// MODE 0 (Go's form) otherwise
int pick_mode(const dsx_ctx* c, uint32_t d) {
  if (c->force_mode >= 0 && c->force_mode <= 2) {
    if (c->force_mode != 2 || (d & (d - 1u)) != 0) return c->force_mode;
  }
  if ((d & (d - 1u)) != 0) return 2;
  return (d > 1024u && d < (1u << 22)) ? 1 : 0;
}

// Stitch segment for a span of n bytes: max(mult * max, floor), doubled while
// the span would have more than seg_target + 1 segments.  An 8 GiB piece gets
// 2 MiB segments (4096-4097 of them): walk 31 + fixup 13.7 + gather 5.0 us
// against 32.5 + 22.5 + 6.8 with 1 MiB, +0.45 % on the bench line; 4 MiB
// lengthens the walks' chains (walk 55.6 us) (profiles/r04k).
uint64_t stitch_seg(const dsx_ctx* c, const dsx_params_t* p, uint64_t n) {
  uint64_t seg = std::max<uint64_t>(c->seg_max_mult * p->max, c->seg_floor);
  if (c->seg_target)
    while ((n + seg - 1) / seg > c->seg_target + 1 && seg < (1ull << 26)) seg <<= 1;
  return seg;
}

// The next scan launch initialises the device chain state (no memcpy).
int reset_state(dsx_ctx* c, uint64_t carry) {
  c->npiece_call = 0;
  c->init_pending = true;
  c->init_carry = carry;
  return DSX_OK;
}

// Wait for the stream; the last fixup_kernel published the state into pinned
// host memory.
int read_state(dsx_ctx* c, HostState* out) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(out, (const void*)c->h_state, sizeof(HostState));
  if (out->seq != c->piece_seq) {
    c->err = "stale chain state (no piece completed)";
    return DSX_E_INTERNAL;
  }
  return DSX_OK;
}

// --------------------------------------------------------------------------
// scan dispatch: which instantiation of dsx_scan.hip a piece's scan launches
// --------------------------------------------------------------------------
// TWO = the piece has two region sizes (ScanArgs.lane_bytes2 != 0); a one-size
// instantiation over a two-size region list reads past the piece, so every
// scanl_kernel row takes TWO from the geometry.  ROTF = DSX_SCAN_ROTF (default
// on).  Rows are tried from the top; the first that applies launches.
//
//   libdsx_diag.so only (launch_scan_diag; variant = DSX_SCAN_VARIANT, cfg =
//   DSX_SCAN_CFG, pf = DSX_PREFETCH > 0):
//     line, behind                scanl_kernel<mode, 0, 8,8,1, true,  false>
//     line, variant 1 3 4 5       scanl_kernel<2, variant, 8,8,1, false, TWO>   (any mode)
//     line, variant 6..10, mode 2 scanl_kernel<2, variant, 8,8,1, false, TWO>
//     rows, variant 1 3 4         scan_kernel<2, variant, CFG>                  (any mode)
//     rows, cfg 1..5, or pf       scan_kernel<mode, 0, CFG>
//       CFG = <BR, NBUF, W, SUB, PF>:  cfg 0  2,2, 8,8,pf    cfg 1  1,2,12,4,false
//         cfg 2  1,2,16,4,false        cfg 3  2,1,12,8,false cfg 4  2,1, 8,8,false
//         cfg 5  2,1,16,4,false
//   (variants 6..10 at mode 0 or 1, variant 2 and any other value fall through
//   to the exact kernels below, as does the behind flag on the row path)
//
//   both libraries:
//     line, ROTF, mode 2          scanl_kernel<2, 0, 8,8,1, false, TWO, true>   (launch_scanl)
//     line                        scanl_kernel<mode, 0, 8,8,1, false, TWO>      (launch_scanl)
//     rows                        scan_kernel<mode, 0, 2,2,8,8,false>           (launch_scan)
using ScanFn = void (*)(ScanArgs);

struct ScanLaunch {
  dim3 grid, block;
  hipStream_t stream;
  const ScanArgs& sa;
  void operator()(ScanFn k) const { hipLaunchKernelGGL(k, grid, block, 0, stream, sa); }
};

template <bool FUSE, bool TWO>
static ScanFn scanl_exact(int mode) {
  switch (mode) {
    case 2: return scanl_kernel<2, 0, 8, 8, 1, FUSE, TWO>;
    case 1: return scanl_kernel<1, 0, 8, 8, 1, FUSE, TWO>;
    default: return scanl_kernel<0, 0, 8, 8, 1, FUSE, TWO>;
  }
}

// the line scan at the product configuration
static void launch_scanl(const ScanLaunch& go, int mode, bool two, bool rotf) {
  if (rotf && mode == 2)  // the rotating frame (MODE 2 only)
    go(two ? scanl_kernel<2, 0, 8, 8, 1, false, true, true> : scanl_kernel<2, 0, 8, 8, 1, false, false, true>);
  else
    go(two ? scanl_exact<false, true>(mode) : scanl_exact<false, false>(mode));
}

template <int BR, int NB, int WV, int SUB, bool PF>
static ScanFn scan_exact(int mode) {
  switch (mode) {
    case 2: return scan_kernel<2, 0, BR, NB, WV, SUB, PF>;
    case 1: return scan_kernel<1, 0, BR, NB, WV, SUB, PF>;
    default: return scan_kernel<0, 0, BR, NB, WV, SUB, PF>;
  }
}

// the 96-B-row scan at the product configuration
static void launch_scan(const ScanLaunch& go, int mode) { go(scan_exact<2, 2, 8, 8, false>(mode)); }

#if DSX_DIAG
template <int V>
static ScanFn scanl_variant(bool two) {
  return two ? scanl_kernel<2, V, 8, 8, 1, false, true> : scanl_kernel<2, V, 8, 8, 1, false, false>;
}

template <int BR, int NB, int WV, int SUB, bool PF>
static ScanFn scan_cfg_of(int mode, int variant) {
  switch (variant) {
    case 1: return scan_kernel<2, 1, BR, NB, WV, SUB, PF>;
    case 3: return scan_kernel<2, 3, BR, NB, WV, SUB, PF>;
    case 4: return scan_kernel<2, 4, BR, NB, WV, SUB, PF>;
    default: return scan_exact<BR, NB, WV, SUB, PF>(mode);
  }
}

// The diagnostic instantiations (the table above); false: none applies, the
// caller launches the exact kernel.
static bool launch_scan_diag(const ScanLaunch& go, bool line, int mode, bool two, int variant,
                             int scan_cfg, bool prefetch, bool behind) {
  ScanFn k = nullptr;
  if (line && behind) {
    k = scanl_exact<true, false>(mode);
  } else if (line) {
    switch (mode == 2 || variant <= 5 ? variant : 0) {
      case 1: k = scanl_variant<1>(two); break;
      case 3: k = scanl_variant<3>(two); break;
      case 4: k = scanl_variant<4>(two); break;
      case 5: k = scanl_variant<5>(two); break;
      case 6: k = scanl_variant<6>(two); break;
      case 7: k = scanl_variant<7>(two); break;
      case 8: k = scanl_variant<8>(two); break;
      case 9: k = scanl_variant<9>(two); break;
      case 10: k = scanl_variant<10>(two); break;
      default: break;
    }
  } else {
    const bool ablate = variant == 1 || variant == 3 || variant == 4;
    switch (scan_cfg) {
      case 1: k = scan_cfg_of<1, 2, 12, 4, false>(mode, variant); break;
      case 2: k = scan_cfg_of<1, 2, 16, 4, false>(mode, variant); break;
      case 3: k = scan_cfg_of<2, 1, 12, 8, false>(mode, variant); break;
      case 4: k = scan_cfg_of<2, 1, 8, 8, false>(mode, variant); break;
      case 5: k = scan_cfg_of<2, 1, 16, 4, false>(mode, variant); break;
      default:
        if (prefetch) k = scan_cfg_of<2, 2, 8, 8, true>(mode, variant);
        else if (ablate) k = scan_cfg_of<2, 2, 8, 8, false>(mode, variant);
    }
  }
  if (k) go(k);
  return k != nullptr;
}
#endif

// --------------------------------------------------------------------------
// enqueue_piece and its parts
// --------------------------------------------------------------------------

// Region lists of a piece: the context's scratch, or (cc.keep: shards) buffers
// of their own that outlive the call, so a re-walk can re-run the stitch
// without scanning the bytes again.
static int region_lists(dsx_ctx* c, const CallCfg& cc, const ScanGeom& g, uint32_t** rcnt,
                        uint32_t** rlist, KeptPiece** kp) {
  if (cc.keep) {
    if (c->sh.nkept == cc.keep->size()) cc.keep->emplace_back();
    *kp = &(*cc.keep)[c->sh.nkept++];
    HIPCHK(c, grow(c, (*kp)->cnt, g.nregions));  // (reused across runs: grows once)
    HIPCHK(c, grow(c, (*kp)->list, g.nregions * g.rcap));
    *rcnt = (*kp)->cnt.p;
    *rlist = (*kp)->list.p;
    return DSX_OK;
  }
  // split streams: two region-list sets, so the next piece's scan writes
  // one while this piece's stitch reads the other
  // (and stitch behind: the next scan writes one while its tasks walk
  // the other)
  const bool split = c->scan_stream != c->stream;
  const bool second = (split || cc.behind) && (c->piece_seq + 1) % 2 == 1;
  auto& bc = second ? c->region_cnt2 : c->region_cnt;
  auto& bl = second ? c->region_list2 : c->region_list;
  HIPCHK(c, grow(c, bc, g.nregions));
  HIPCHK(c, grow(c, bl, g.nregions * g.rcap));
  *rcnt = bc.p;
  *rlist = bl.p;
  return DSX_OK;
}

#if DSX_DIAG
// The pending jobs of the calls behind: the walk of the one not walked yet,
// the finish of the one that is.
static void behind_tasks(const dsx_ctx* c, TaskArgs* tb) {
  for (const auto& b : c->behind) {
    if (!b.walked) {
      tb->w = b.w;
      tb->nw = b.nw;
      tb->wseg = b.wseg;
    } else {
      tb->f = b.f;
      tb->nf = b.nf;
      tb->fseg = b.fseg;
    }
  }
}

// Those jobs are launched: the walked call is done, the other one is walked
// now, and `me` (if any) joins behind them.
static void behind_rotate(dsx_ctx* c, const dsx_ctx::Behind* me = nullptr) {
  std::deque<dsx_ctx::Behind> next;
  for (auto& b : c->behind)
    if (!b.walked) {
      b.walked = true;
      next.push_back(b);
    }
  if (me) next.push_back(*me);
  c->behind.swap(next);
}

// Stitch behind: this call's segment set (by piece parity) and its walk and
// finish jobs, but for the candidate lists and the seq (known after the scan
// is set up).
static int behind_jobs(dsx_ctx* c, const CallCfg& cc, uint64_t len, dsx_ctx::Behind* me) {
  const dsx_params_t* p = cc.p;
  const bool second = (c->piece_seq + 1) % 2 == 1;
  const uint64_t seg = stitch_seg(c, p, len);
  const uint64_t nseg = (len + seg - 1) / seg;
  const uint32_t scap = (uint32_t)(seg / p->min + 3);
  auto& bs = second ? c->seg_info2 : c->seg_info;
  auto& bt = second ? c->stage2 : c->stage;
  auto& bp = second ? c->spec2 : c->spec;
  if (bs.n < nseg || bt.n < nseg * scap || bp.n < nseg * scap) {
    // the call two back may still have to finish from this set: launch it
    // on its own before the set is reallocated
    int rc = flush_behind(c);
    if (rc) return rc;
    HIPCHK(c, grow(c, bs, nseg));
    HIPCHK(c, grow(c, bt, nseg * scap));
    HIPCHK(c, grow(c, bp, nseg * scap));
  }
  // segments per walk task (one lane each, up to 63): the task's
  // candidates fill at most half of its LDS on average
  const double exp_per_seg = (double)seg / (double)p->discriminator + 8.0;
  me->wseg = (uint32_t)std::max(1.0, std::min(32.0, std::floor(kTaskCand / (2.0 * exp_per_seg)) - 1.0));
  me->fseg = 32;
  me->nw = (uint32_t)((nseg + me->wseg - 1) / me->wseg);
  me->nf = (uint32_t)((nseg + me->fseg - 1) / me->fseg);
  me->w.min = p->min;
  me->w.max = p->max;
  me->w.L = len;
  me->w.seg = seg;
  me->w.nseg = (uint32_t)nseg;
  me->w.scap = scap;
  me->w.seg_info = bs.p;
  me->w.stage = bt.p;
  me->w.spec = bp.p;
  me->f.seg_info = bs.p;
  me->f.stage = bt.p;
  me->f.spec = bp.p;
  me->f.nseg = (uint32_t)nseg;
  me->f.scap = scap;
  me->f.out = cc.d_out;
  me->f.out_cap = cc.out_cap;
  me->f.host_state = c->h_cur;
  return DSX_OK;
}
#endif

// What scan_geom reads of the piece, the call and the context's settings.
static ScanGeomIn geom_in(const dsx_ctx* c, const CallCfg& cc, const uint8_t* d_piece,
                          uint64_t halo, uint64_t P, uint64_t len) {
  ScanGeomIn gi;
  gi.len = len;
  gi.P = P;
  gi.halo = halo;
  gi.delta = (uint32_t)((uintptr_t)d_piece & (kLine - 1));
  gi.discriminator = cc.p->discriminator;
  gi.dense = cc.dense;
  gi.behind = cc.behind;
  gi.scan_line = c->scan_line;
  gi.scan_cfg = c->scan_cfg;
  gi.scanl_waves = c->scanl_waves;
  gi.ncu = c->ncu;
  gi.stitch_cus = c->stitch_cus;
  gi.split = c->scan_stream != c->stream;
  gi.regions_per_slot = c->regions_per_slot;
  gi.lane_target = c->lane_target;
  gi.lane_bytes_override = c->lane_bytes_override;
  gi.tail_split = c->tail_split;
  gi.tail_mult = c->tail_mult;
  return gi;
}

// DSX_SCAN_TRACE: the piece's (zeroed) trace slot, for the scan's per-wave
// records and the walk records after them.
static int trace_slot(dsx_ctx* c, bool behind, int W, uint64_t seq, hipStream_t ss, uint64_t** out) {
  c->trace_n = (uint64_t)c->ncu * W;
  const uint64_t slot_words = kScanTraceWords * c->trace_n + 10 * 65536ull;
  HIPCHK(c, grow(c, c->trace, (c->trace_keep ? 4 : 1) * slot_words));
  c->trace_base = c->trace_keep ? (seq % 4) * slot_words : 0;
  // (stitch behind: 6 task words per wave slot follow, read as walk records)
  const uint64_t tw = behind ? 6 * c->trace_n : 0;
  HIPCHK(c, hipMemsetAsync(c->trace.p + c->trace_base, 0, (kScanTraceWords * c->trace_n + tw) * sizeof(uint64_t), ss));
  *out = c->trace.p + c->trace_base;
  if (behind) c->trace_walk_n = (tw + 9) / 10;
  return DSX_OK;
}

// Enqueue the scan of one piece [P, P+len) whose bytes are at d_piece (with
// `halo` readable bytes before it).  so->pc: the piece's candidate lists as a
// stitch reads them (on the ctx stream, which waits for the scan).
int enqueue_scan(dsx_ctx* c, const CallCfg& cc, const uint8_t* d_piece, uint64_t halo, uint64_t P,
                 uint64_t len, ScanOut* so, const TaskArgs* behind_tb) {
  const dsx_params_t* p = cc.p;
  const bool split = c->scan_stream != c->stream;
  const ScanGeom g = scan_geom(geom_in(c, cc, d_piece, halo, P, len));
  const bool line = g.line;
  HIPCHK(c, grow(c, c->lane_slot, g.nlanes * g.LS));
  uint32_t *rcnt = nullptr, *rlist = nullptr;
  KeptPiece* kp = nullptr;
  int rc = region_lists(c, cc, g, &rcnt, &rlist, &kp);
  if (rc) return rc;
  const uint64_t seq = ++c->piece_seq;
  const int par = (int)(seq & 1);
  hipStream_t ss = c->scan_stream;

  ScanArgs sa{};
  sa.base = d_piece;
  sa.halo = halo;
  sa.piece_abs = P;
  sa.len = len;
  sa.lane_bytes = g.S;
  sa.batches = g.batches;
  sa.nregions = (uint32_t)g.nregions;
  if (g.S2) {
    sa.nbig = (uint32_t)g.nbig;
    sa.lane_bytes2 = (uint32_t)g.S2;
    sa.batches2 = g.batches2;
  }
  sa.region_cap = g.rcap;
  sa.tc = make_tc(p);
  sa.min_pos = cc.min_pos;
  sa.lane_slots = g.LS;
  sa.pf_batches = (uint32_t)c->prefetch_batches;
  sa.lane_slot = c->lane_slot.p;
  sa.region_cnt = rcnt;
  sa.region_list = rlist;
  // overflow word and queue counters: slot seq % 4; the scan zeroes the next
  // piece's slot (the stitch of the previous piece may still read its own)
  sa.overflow = c->overflow.p + (seq % kQueueSlots);
  sa.overflow_next = c->overflow.p + ((seq + 1) % kQueueSlots);
  sa.queue = c->overflow.p + 32 + 256 * (seq % kQueueSlots);
  sa.queue_next = c->overflow.p + 32 + 256 * ((seq + 1) % kQueueSlots);
  sa.delta = g.delta;
  sa.shift0 = g.shift0;
  sa.wave_major = c->wave_major ? (cc.behind ? 2u : 1u) : 0u;
  sa.nt_loads = (uint32_t)c->scan_nt;
  if (c->pub_host) {  // the previous queued piece's state, published by this scan
    sa.pub_state = c->state.p;
    sa.pub_host = c->pub_host;
    sa.pub_seq = c->pub_seq;
    c->pub_host = nullptr;
  }
#if DSX_DIAG
  if (behind_tb) {
    TaskArgs tb = *behind_tb;
    tb.counter = sa.queue + 1;  // (zeroed by the previous scan, with the queue)
    tb.farrive = sa.queue + 2;
    // the ring advances with fused calls only: the slot was last read by the
    // scan of the fused call kTaskRing (16) fused calls ago, which completed
    // before the call kQueueDepth (8) queued calls ago was collected (a
    // non-fused multi-piece call between them does not move the index)
    TaskArgs* slot = c->h_tasks + (c->fuse_seq++ % dsx_ctx::kTaskRing);
    *slot = tb;
    sa.tasks = slot;
  }
#endif
  if (c->stamping && line && c->stamp_meta.size() < c->stamp_cap && g.W == c->scanl_waves) {
    sa.stamp = c->stamp_ring.p + c->stamp_slots * kStampWords * c->stamp_meta.size();
    c->stamp_meta.emplace_back(seq, len);
  }
  if (c->scan_trace && line) {
    rc = trace_slot(c, cc.behind, g.W, seq, ss, &sa.trace);
    if (rc) return rc;
  }
  const uint32_t pi = c->npiece_call++;
  while (c->pev.size() < 3 * (size_t)(pi + 1)) {
    hipEvent_t e;
    HIPCHK(c, hipEventCreate(&e));
    c->pev.push_back(e);
  }
  // the region lists this scan writes were read by the stitch two pieces ago
  if (split) HIPCHK(c, hipStreamWaitEvent(ss, c->ev_stitch[par], 0));
  if (c->timing) HIPCHK(c, hipEventRecord(c->pev[3 * pi], ss));
#if DSX_DIAG
  if (getenv("DSX_NOOP_BEFORE_SCAN")) hipLaunchKernelGGL(noop_kernel, dim3(1), dim3(64), 0, ss);
#endif
  {
    const ScanLaunch go{dim3(g.grid), dim3(g.W * kWave), ss, sa};
    const int mode = pick_mode(c, p->discriminator);
    const bool two = sa.lane_bytes2 != 0;
#if DSX_DIAG
    if (!launch_scan_diag(go, line, mode, two, c->variant, c->scan_cfg, c->prefetch_batches > 0,
                          cc.behind))
#endif
    {
      if (line) launch_scanl(go, mode, two, c->scan_rotf);
      else launch_scan(go, mode);
    }
    HIPCHK(c, hipGetLastError());
  }
  if (c->timing) HIPCHK(c, hipEventRecord(c->pev[3 * pi + 1], ss));
  if (split) {  // the stitch (ctx stream) after the scan (scan stream)
    HIPCHK(c, hipEventRecord(c->ev_scan[par], ss));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_scan[par], 0));
  }
  PieceCands pc{};
  pc.P = g.grid_P;  // region r covers (P' + base(r), P' + base(r) + bytes(r)]
  pc.RB = g.region_bytes;
  pc.RB2 = g.region_bytes2;
  pc.nbig = (uint32_t)g.nbig;
  pc.nregions = (uint32_t)g.nregions;
  pc.region_cap = g.rcap;
  pc.region_cnt = rcnt;
  pc.region_list = rlist;
  pc.overflow = sa.overflow;
  if (kp) {
    kp->pc = pc;
    kp->P = P;
    kp->len = len;
  }
  so->pc = pc;
  so->seq = seq;
  so->pi = pi;
  so->line = line;
  return DSX_OK;
}

// Enqueue scan + stitch for one piece [P, P+len) whose bytes are at d_piece
// (with `halo` readable bytes before it).  *pc_out: the piece's candidate
// lists as the stitch reads them.
int enqueue_piece(dsx_ctx* c, const CallCfg& cc, const uint8_t* d_piece, uint64_t halo,
                  uint64_t P, uint64_t len, bool is_last, PieceCands* pc_out) {
  const bool split = c->scan_stream != c->stream;
  int rc;
  ScanOut so;
  // stitch behind: this call's jobs, and the tasks of the calls behind it
  // that this scan carries
#if DSX_DIAG
  TaskArgs tb{};
  dsx_ctx::Behind me;
  if (cc.behind) {
    rc = behind_jobs(c, cc, len, &me);
    if (rc) return rc;
    behind_tasks(c, &tb);
  }
  rc = enqueue_scan(c, cc, d_piece, halo, P, len, &so, cc.behind ? &tb : nullptr);
#else
  rc = enqueue_scan(c, cc, d_piece, halo, P, len, &so);
#endif
  if (rc) return rc;
  const uint32_t pi = so.pi;
  const int par = (int)(so.seq & 1);
  if (pc_out) *pc_out = so.pc;
#if DSX_DIAG
  if (cc.behind) {
    // the call two back finished in this scan, the last one walked in it;
    // this one waits for the next scan (or flush_behind)
    me.w.pc = so.pc;
    me.f.overflow = so.pc.overflow;
    me.f.seq = so.seq;
    me.seq = so.seq;
    behind_rotate(c, &me);
    c->init_pending = false;
    c->last_finish = false;
    if (c->timing) HIPCHK(c, hipEventRecord(c->pev[3 * pi + 2], c->stream));
    c->stats.pieces++;
    return DSX_OK;
  }
#endif
  rc = launch_stitch(c, cc, so.pc, P, len, is_last, so.seq, so.line && c->scan_trace);
  if (rc) return rc;
  if (split) HIPCHK(c, hipEventRecord(c->ev_stitch[par], c->stream));
  if (c->timing) HIPCHK(c, hipEventRecord(c->pev[3 * pi + 2], c->stream));
  c->stats.pieces++;
  return DSX_OK;
}

// The piece's state into the pinned host slot after its stitch (the host
// polls it for queued calls, reads it after a sync otherwise).
static int launch_publish(dsx_ctx* c, const StitchArgs& ta) {
  c->last_finish = ta.host_state != nullptr;
  if (!ta.host_state) return DSX_OK;
  if (c->defer_publish) {  // a queued call: the next scan publishes it
    c->pub_host = ta.host_state;
    c->pub_seq = ta.seq;
    return DSX_OK;
  }
  hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, c->stream, ta);
  HIPCHK(c, hipGetLastError());
  return DSX_OK;
}

int flush_publish(dsx_ctx* c) {
  if (!c->pub_host) return DSX_OK;
  StitchArgs ta{};
  ta.state = c->state.p;
  ta.host_state = c->pub_host;
  ta.seq = c->pub_seq;
  c->pub_host = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, c->stream, ta);
  HIPCHK(c, hipGetLastError());
  return DSX_OK;
}

// walk -> fixup -> gather for one piece whose candidates are in pc.
int launch_stitch(dsx_ctx* c, const CallCfg& cc, const PieceCands& pc, uint64_t P, uint64_t len,
                  bool is_last, uint64_t seq, bool trace) {
  const dsx_params_t* p = cc.p;
  const uint64_t region_bytes = pc.RB;
  StitchArgs ta{};
  ta.chain.min = p->min;
  ta.chain.max = p->max;
  ta.chain.L = cc.L;
  ta.chain.PE = P + len;
  ta.chain.is_last = is_last ? 1u : 0u;
  ta.pc = pc;
  // the carried cut lies in (P - max, P] (its successor needed bytes >= P)
  const uint64_t anchor = (P > cc.origin + p->max) ? P - p->max : cc.origin;
  const uint64_t end = is_last ? cc.L : P + len;
  const uint64_t seg = stitch_seg(c, p, end > anchor ? end - anchor : 1);
  const uint64_t nseg = end > anchor ? (end - anchor + seg - 1) / seg : 1;
  ta.anchor = anchor;
  ta.seg = seg;
  ta.nseg = (uint32_t)nseg;
  const double exp_per_seg = (double)seg / (double)p->discriminator + 8.0;
  // segments per walk workgroup: about two workgroups per CU (the walks are
  // latency-bound), within the LDS candidate and region budgets
  uint64_t spg = std::max<uint64_t>(2, nseg / ((uint64_t)c->walk_wgs * (uint64_t)c->ncu));
  // split streams: the walk runs beside the next piece's scan on the CUs the
  // scan leaves free, two 1024-thread workgroups per CU (LDS: ~69 KiB each)
  const bool wide = c->scan_stream != c->stream;
  if (wide)
    spg = std::max<uint64_t>(spg, (nseg + 2ull * c->stitch_cus - 1) / (2ull * c->stitch_cus));
  spg = std::min<uint64_t>(spg, (uint64_t)((double)kWalkLdsCap / (2.0 * exp_per_seg)) - 1);
  // (the smaller region size bounds the regions a workgroup's span covers:
  // two region sizes put the short tail regions at the piece's end)
  const uint64_t rb_min = pc.RB2 ? std::min<uint64_t>(region_bytes, pc.RB2) : region_bytes;
  const uint64_t max_spg_reg = rb_min ? (4000ull * rb_min) / seg : kMaxSpg;
  spg = std::min<uint64_t>(spg, max_spg_reg > 2 ? max_spg_reg - 2 : 1);
  spg = std::max<uint64_t>(1, std::min<uint64_t>(spg, kMaxSpg));
  ta.spg = (uint32_t)spg;
  ta.lds_cap = kWalkLdsCap;
  ta.scap = (uint32_t)(seg / p->min + 3);
  HIPCHK(c, grow(c, c->seg_info, nseg));
  HIPCHK(c, grow(c, c->stage, nseg * ta.scap));
  HIPCHK(c, grow(c, c->rep, nseg * ta.scap));
  HIPCHK(c, grow(c, c->rep_cnt, nseg));
  HIPCHK(c, grow(c, c->rep_from, nseg));
  HIPCHK(c, grow(c, c->flag_list, nseg));
  HIPCHK(c, grow(c, c->out_off, nseg));
  ta.seg_info = c->seg_info.p;
  ta.stage = c->stage.p;
  ta.rep = c->rep.p;
  ta.rep_cnt = c->rep_cnt.p;
  ta.rep_from = c->rep_from.p;
  ta.flag_list = c->flag_list.p;
  ta.out_off = c->out_off.p;
  ta.out = cc.d_out;
  ta.out_cap = cc.out_cap;
  ta.state = c->state.p;
  ta.host_state = c->h_cur;
  ta.seq = seq;
  ta.init = c->init_pending ? 1u : 0u;  // the call's first piece: walk_kernel resets the state
  ta.init_carry = c->init_carry;
  c->init_pending = false;
  c->last_finish = false;
  const uint32_t walk_grid = (uint32_t)((nseg + spg - 1) / spg);
  if (trace && walk_grid <= 65536) {
    ta.trace = c->trace.p + c->trace_base + kScanTraceWords * c->trace_n;
    c->trace_walk_n = walk_grid;
  }
  const size_t walk_lds = (size_t)kWalkLdsCap * 4 + (kMaxSpg + 1) * 8;
  if (wide)
    hipLaunchKernelGGL(walk_kernel<1024>, dim3(walk_grid), dim3(1024), walk_lds, c->stream, ta);
  else if (c->walk_nt == 576 && spg == 8)  // (the 8 GiB pieces: 8 segments + the redundant one, a wave each)
    hipLaunchKernelGGL(walk_kernel<576>, dim3(walk_grid), dim3(576), walk_lds, c->stream, ta);
  else
    hipLaunchKernelGGL(walk_kernel<256>, dim3(walk_grid), dim3(256), walk_lds, c->stream, ta);
  HIPCHK(c, hipGetLastError());
  if (c->finish && nseg <= 2048) {  // fixup + gather over nseg/16 workgroups
    const dim3 fg((uint32_t)((nseg + 15) / 16));
    if (nseg <= 256) hipLaunchKernelGGL(finish_kernel<1>, fg, dim3(256), 0, c->stream, ta);
    else if (nseg <= 512) hipLaunchKernelGGL(finish_kernel<2>, fg, dim3(256), 0, c->stream, ta);
    else if (nseg <= 1024) hipLaunchKernelGGL(finish_kernel<4>, fg, dim3(256), 0, c->stream, ta);
    else hipLaunchKernelGGL(finish_kernel<8>, fg, dim3(256), 0, c->stream, ta);
    HIPCHK(c, hipGetLastError());
    return launch_publish(c, ta);
  }
  if (c->fixup_fast && nseg <= 9 * 1024) {
    if (nseg <= 1024) hipLaunchKernelGGL(fixup_fast_kernel<1>, dim3(1), dim3(1024), 0, c->stream, ta);
    else if (nseg <= 2048) hipLaunchKernelGGL(fixup_fast_kernel<2>, dim3(1), dim3(1024), 0, c->stream, ta);
    else if (nseg <= 4096) hipLaunchKernelGGL(fixup_fast_kernel<4>, dim3(1), dim3(1024), 0, c->stream, ta);
    else if (nseg <= 5120) hipLaunchKernelGGL(fixup_fast_kernel<5>, dim3(1), dim3(1024), 0, c->stream, ta);
    else if (nseg <= 8192) hipLaunchKernelGGL(fixup_fast_kernel<8>, dim3(1), dim3(1024), 0, c->stream, ta);
    else hipLaunchKernelGGL(fixup_fast_kernel<9>, dim3(1), dim3(1024), 0, c->stream, ta);
  } else {
    hipLaunchKernelGGL(fixup_kernel, dim3(1), dim3(1024), 0, c->stream, ta);
  }
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(gather_kernel, dim3((uint32_t)nseg), dim3(256), 0, c->stream, ta);
  HIPCHK(c, hipGetLastError());
  return launch_publish(c, ta);
}

// Runs a whole device-resident blob [origin.., origin+len) through the engine.
int run_device(dsx_ctx* c, const uint8_t* d_blob, uint64_t len, CallCfg cc) {
  HIPCHK(c, hipSetDevice(c->device));
  int rc = reset_state(c, cc.origin);
  if (rc) return rc;
  const uint64_t piece = cc.dense ? kDensePiece : kPieceMax;
  for (uint64_t off = 0; off < len; off += piece) {
    if (c->cancel.load()) return DSX_E_INTERRUPTED;
    const uint64_t n = std::min(piece, len - off);
    rc = enqueue_piece(c, cc, d_blob + off, off + cc.halo0, cc.origin + off, n, off + n == len);
    if (rc) return rc;
  }
  return DSX_OK;
}

int ensure_attr_walk(dsx_ctx* c) {
  static bool done = false;
  if (!done) {
    HIPCHK(c, hipFuncSetAttribute((const void*)walk_kernel<256>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kWalkLdsCap * 4 + (kMaxSpg + 1) * 8)));
    HIPCHK(c, hipFuncSetAttribute((const void*)walk_kernel<576>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kWalkLdsCap * 4 + (kMaxSpg + 1) * 8)));
    HIPCHK(c, hipFuncSetAttribute((const void*)walk_kernel<1024>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kWalkLdsCap * 4 + (kMaxSpg + 1) * 8)));
    done = true;
  }
  return DSX_OK;
}

int flush_behind(dsx_ctx* c) {
  const int rc = flush_tasks(c);
  return rc ? rc : flush_publish(c);
}

int flush_tasks(dsx_ctx* c) {
  if (c->behind.empty()) return DSX_OK;
#if DSX_DIAG
  HIPCHK(c, hipSetDevice(c->device));
  // round 1: the walked call's finish and the other's walk (independent);
  // round 2: the latter's finish
  while (!c->behind.empty()) {
    TaskArgs tb{};
    tb.farrive = c->overflow.p + kArriveWord + 1;
    behind_tasks(c, &tb);
    const uint32_t n = tb.nw + tb.nf;
    if (n) {
      hipLaunchKernelGGL(stitch_task_kernel, dim3((n + 3) / 4), dim3(256), 0, c->stream, tb);
      HIPCHK(c, hipGetLastError());
    }
    behind_rotate(c);
  }
#endif
  return DSX_OK;
}

// --------------------------------------------------------------------------
// many blobs in one packed buffer (dsx_cut_device_many)
// --------------------------------------------------------------------------
// The batched walk's positions are 32-bit offsets from a run's start, and a
// step of max (clamped to 2^30) must stay in them: a longer blob is single.
constexpr uint64_t kManyMaxBatched = 1ull << 30;
constexpr uint32_t kManyRunBlobs = 4096;  // blobs per walk workgroup (16 rounds of its 4 waves)
static_assert(sizeof(ManyRun) == sizeof(ManyRunDev), "the plan's runs are uploaded as they are");
static_assert(kManyLdsCap == kWalkLdsCap, "the batched walk stages what walk_kernel stages");

// The length whose expected candidate count (len / discriminator + 8) is half
// of what a walk workgroup stages: longer blobs take the one-blob path.
uint64_t many_default_big_blob(const dsx_params_t* p) {
  return std::min<uint64_t>(kManyMaxBatched, (uint64_t)(kWalkLdsCap / 2 - 8) * p->discriminator);
}

// Blob i = [B0, B1) on the one-blob path (run_device, with the dense retry of
// dsx_cut_device), its cuts into its slots of the staging list.
static int many_single(dsx_ctx* c, const uint8_t* d_blob, const ManyBlobs& mb,
                       const dsx_params_t* p, uint64_t i, uint64_t B0, uint64_t B1) {
  const uint64_t slots = (B1 - B0) / p->min + 1;
  for (int attempt = 0; attempt < 2; ++attempt) {
    CallCfg cc{p, B1, B0, B0 + kRound, mb.stage + (B0 / p->min + i), slots, attempt == 1};
    cc.halo0 = B0;
    int rc = run_device(c, d_blob + B0, B1 - B0, cc);
    if (rc) return rc;
    HostState s;
    rc = read_state(c, &s);
    if (rc) return rc;
    if (s.err & kErrDense) {
      c->stats.dense_fallbacks++;
      continue;
    }
    if ((s.err & kErrCapacity) || s.total > slots) {
      c->err = "a blob has more cuts than its slots of the staging list";
      return DSX_E_INTERNAL;
    }
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(mb.cnt + i), (int)s.total, 1, c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(mb.flag + i), 0, 1, c->stream));
    return DSX_OK;
  }
  c->err = "dense-candidate path overflowed";
  return DSX_E_INTERNAL;
}

// One group: a scan launch over its bytes, then the batched walk.
static int many_group(dsx_ctx* c, const uint8_t* d_blob, const ManyBlobs& mb, const dsx_params_t* p,
                      const uint64_t* blob_ends, const ManyItem& it, std::vector<ManyRun>* runs) {
  const bool split = c->scan_stream != c->stream;
  // chain origin = the group's start; the bytes before it in the packed
  // buffer are its halo (a group off the 128-byte grid keeps the line scan)
  CallCfg cc{p, it.end, it.start, it.start + kRound, nullptr, 0, false};
  c->npiece_call = 0;  // (no timing events: the groups are not pieces of a chain)
  const bool timing = c->timing;
  c->timing = false;
  ScanOut so;
  const int rc = enqueue_scan(c, cc, d_blob + it.start, it.start, it.start, it.end - it.start, &so);
  c->timing = timing;
  if (rc) return rc;
  // blobs per walk workgroup: expected candidates within half of its LDS, the
  // regions it can stage, and enough workgroups for the device
  const PieceCands& pc = so.pc;
  const uint64_t rb_min = pc.RB2 ? std::min<uint64_t>(pc.RB, pc.RB2) : pc.RB;
  uint64_t span = (uint64_t)(kWalkLdsCap / 2 - 8) * p->discriminator;
  if (rb_min) span = std::min<uint64_t>(span, 3998ull * rb_min);
  span = std::min<uint64_t>(span, kManyMaxBatched);
  span = std::min<uint64_t>(span, std::max<uint64_t>((it.end - it.start) / (4ull * c->ncu), 256ull << 10));
  many_runs(blob_ends, it.b0, it.b1, span, kManyRunBlobs, runs);
  HIPCHK(c, grow(c, c->many.runs, runs->size()));
  HIPCHK(c, hipMemcpyAsync(c->many.runs.p, runs->data(), runs->size() * sizeof(ManyRun),
                           hipMemcpyHostToDevice, c->stream));
  ManyWalkArgs wa{};
  wa.mb = mb;
  wa.pc = pc;
  wa.runs = c->many.runs.p;
  wa.lds_cap = kWalkLdsCap;
  hipLaunchKernelGGL(many_walk_kernel, dim3((uint32_t)runs->size()), dim3(kManyWalkThreads), 0,
                     c->stream, wa);
  HIPCHK(c, hipGetLastError());
  if (split) HIPCHK(c, hipEventRecord(c->ev_stitch[so.seq & 1], c->stream));
  return DSX_OK;
}

int run_many(dsx_ctx* c, const uint8_t* d_blob, uint64_t len, const uint64_t* blob_ends,
             uint64_t nblobs, const dsx_params_t* p, uint64_t* out_ends, uint64_t cap,
             uint64_t* n_out, uint64_t* blob_first, uint64_t big_blob, uint64_t group_bytes,
             dsx_many_totals_t* totals, bool dev_out) {
  HIPCHK(c, hipSetDevice(c->device));
  big_blob = std::min<uint64_t>(big_blob, kManyMaxBatched);
  const std::vector<ManyItem> items = many_plan(blob_ends, nblobs, big_blob, group_bytes);
  auto& m = c->many;
  HIPCHK(c, grow(c, m.ends, nblobs));
  HIPCHK(c, grow(c, m.stage, len / p->min + nblobs + 1));
  HIPCHK(c, grow(c, m.cnt, 2 * nblobs));
  HIPCHK(c, grow(c, m.first, nblobs + 1));
  HIPCHK(c, grow(c, m.res, 2));
  HIPCHK(c, hipMemcpyAsync(m.ends.p, blob_ends, nblobs * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(m.cnt.p, 0, 2 * nblobs * sizeof(uint32_t), c->stream));
  ManyBlobs mb{};
  mb.ends = m.ends.p;
  mb.stage = m.stage.p;
  mb.cnt = m.cnt.p;
  mb.flag = m.cnt.p + nblobs;
  mb.nblobs = nblobs;
  mb.min = p->min;
  mb.max = p->max;

  dsx_many_totals_t t{};
  t.blobs = nblobs;
  std::deque<std::vector<ManyRun>> runs;  // (kept until the call's last wait)
  for (const ManyItem& it : items) {
    if (c->cancel.load()) return DSX_E_INTERRUPTED;
    uint64_t nonempty = 0;
    for (uint64_t i = it.b0; i < it.b1; ++i) nonempty += blob_ends[i] != (i ? blob_ends[i - 1] : 0);
    t.empty_blobs += it.b1 - it.b0 - nonempty;
    if (it.end == it.start) continue;  // nothing but empty blobs
    int rc;
    if (it.single) {
      rc = many_single(c, d_blob, mb, p, it.big, it.start, it.end);
      t.single_blobs++;
    } else {
      runs.emplace_back();
      rc = many_group(c, d_blob, mb, p, blob_ends, it, &runs.back());
      t.groups++;
      t.batched_blobs += nonempty;
    }
    if (rc) return rc;
  }

  ManyFinishArgs fa{};
  fa.mb = mb;
  fa.first = m.first.p;
  fa.res = m.res.p;
  uint64_t res[2] = {0, 0};
  for (int round = 0; round < 2; ++round) {
    hipLaunchKernelGGL(many_scan_kernel, dim3(1), dim3(kManyScanThreads), 0, c->stream, fa);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(res, m.res.p, sizeof(res), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!res[1]) break;
    if (round == 1) {
      c->err = "blobs still flagged after the one-blob path";
      return DSX_E_INTERNAL;
    }
    // the batched walk could not hold these blobs (their candidates did not
    // fit its LDS, or the group's scan overflowed a lane): the one-blob path
    std::vector<uint32_t> flag(nblobs);
    HIPCHK(c, hipMemcpy(flag.data(), mb.flag, nblobs * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < nblobs; ++i) {
      if (!flag[i]) continue;
      if (c->cancel.load()) return DSX_E_INTERRUPTED;
      const int rc = many_single(c, d_blob, mb, p, i, i ? blob_ends[i - 1] : 0, blob_ends[i]);
      if (rc) return rc;
      t.redone_blobs++;
    }
  }
  t.chunks = res[0];
  if (totals) *totals = t;
  *n_out = res[0];
  if (res[0] > cap) return DSX_E_CAPACITY;
  if (res[0]) {
    if (!dev_out) HIPCHK(c, grow(c, c->out, res[0]));
    fa.out = dev_out ? out_ends : c->out.p;
    hipLaunchKernelGGL(many_gather_kernel,
                       dim3((uint32_t)((nblobs + kManyGatherThreads - 1) / kManyGatherThreads)),
                       dim3(kManyGatherThreads), 0, c->stream, fa);
    HIPCHK(c, hipGetLastError());
    if (!dev_out)
      HIPCHK(c, hipMemcpyAsync(out_ends, c->out.p, res[0] * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  }
  if (blob_first)
    HIPCHK(c, hipMemcpyAsync(blob_first, m.first.p, (nblobs + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stats.chunks = res[0];
  return DSX_OK;
}
