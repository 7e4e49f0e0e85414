"""The seam record of dsx_shard_local against oracle/seam.py, field by field.

Every other GPU test of the scan compares a final cut list with the oracle's,
and a cut list shows only the candidates the chain landed on: a quarter of
the positions with h % d == d-1 lie within `min` of the previous cut and are
never one.  dsx_seam_t.cands[] is the scan's own candidate list (every
candidate of the shard's first window, seam_cands_kernel reads it from the
scan's region lists), so here it is the observable:

1. records at the window's truncation branches (the 1024-candidate cap, the
   1024-cut cap, a window shorter than 32*max, the empty shard, the dense
   path), as host records, device records and through the asynchronous path,
   and a shard that ends inside the blob off the 4-byte grid;
2. every candidate of a 64 MiB blob, by tiling it with windows: the next
   shard starts at (or just before) the last record's window_end, under
   DSX_SCAN_ROTF=1 and =0, whose records must hold the same bytes;
3. the protocol end to end where windows are truncated and where seams do not
   converge, every round's records and outcome against oracle/seam.py.

Position origin + 48 is the one position left out: the scan drops p < origin
+ 49, oracle/seam.py keeps p >= 48, and no chain can use p <= origin + min.
Every input used with start == 0 is asserted to have no candidate there.

Out of reach of a record: the two-size tail regions start about 3 GiB into a
piece and a window sees only a piece's first 32*max bytes, so the 4 GiB
cut-list cases (test_gpu_rotframe.py, test_gpu_variants.py) remain the only
check of those regions.  The next gap: stream and dsx_index_* batches, whose
candidates no ABI call exposes.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as o
from oracle import seam as oseam

pytestmark = pytest.mark.gpu

DEFAULT = (16 << 10, 64 << 10, 256 << 10)
MID = (1024, 4096, 16384)
SMALL = (48, 256, 8192)
U64_MAX = 2**64 - 1
NCAP = 1024  # DSX_SEAM_MAX_CANDS == DSX_SEAM_MAX_CUTS
HOST, DEVICE, ASYNC = "host", "device", "async"
VARIANTS = (HOST, DEVICE, ASYNC)


def torch_dev(arr):
    import torch
    t = torch.from_numpy(np.array(arr, dtype=np.uint8, copy=True)).to("cuda")
    torch.cuda.synchronize()
    return t


def _params(mn, av, mx):
    import desync_amd
    return desync_amd.Params(mn, av, mx)


def _flags(variant):
    from desync_amd import _lib
    return {HOST: 0, DEVICE: _lib.DSX_SEAM_DEVICE,
            ASYNC: _lib.DSX_SEAM_DEVICE | _lib.DSX_NO_SYNC}[variant]


def _read_back(ctx, rec):
    """A device record's bytes as a _lib.Seam, once the context's stream is idle."""
    from desync_amd import _lib
    _lib.check(_lib.lib().dsx_sync(ctx.h), ctx.h)
    return _lib.Seam.from_buffer_copy(rec.cpu().numpy().tobytes())


def record(ctx, t, start, length, total, params, flags):
    """dsx_shard_local on the shard [start, start + length) of the device blob
    t; returns the record as a _lib.Seam (a device record is copied back
    after dsx_sync)."""
    import torch
    from desync_amd import _lib, shard
    if flags & _lib.DSX_SEAM_DEVICE:
        rec = torch.full((shard.SEAM_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ptr = rec.data_ptr()
    else:
        rec = _lib.Seam()
        ptr = ctypes.addressof(rec)
    _lib.check(_lib.lib().dsx_shard_local(ctx.h, ctypes.c_void_p(t.data_ptr() + start),
                                          64 if start else 0, start, length, total,
                                          ctypes.byref(params.c), ctypes.c_void_p(ptr), flags), ctx.h)
    return _read_back(ctx, rec) if flags & _lib.DSX_SEAM_DEVICE else rec


def expect(data, start, length, total, mn, av, mx, cands=None):
    """oracle/seam.py's record of the shard, with the first_cand_beyond the
    code stores: the 1025th candidate of (start, start + min(length, 32*max)],
    else 2^64-1.  Returns (record, the shard's chain, its candidates)."""
    seam, cuts, c = oseam.shard_local(data, start, length, total, mn, av, mx, cands=cands)
    w = c[c <= start + min(length, 32 * mx)]
    seam["first_cand_beyond"] = int(w[NCAP]) if w.size > NCAP else U64_MAX
    return seam, cuts, c


def _first_diff(got, want, start, what):
    for i in range(max(len(got), len(want))):
        g = got[i] if i < len(got) else None
        w = want[i] if i < len(want) else None
        if g != w:
            p = min(x for x in (g, w) if x is not None)
            kind = "spurious" if p == g else "missing"
            return (f"{what}[{i}]: got {g}, oracle {w}: {kind} {p} = start + {p - start}, "
                    f"(p - start) % 384 = {(p - start) % 384}, % 128 = {(p - start) % 128}")
    return None


def mismatches(rec, exp, start):
    """The fields of the record `rec` (_lib.Seam) that differ from the oracle
    record `exp` (dict), as messages; empty when they agree."""
    msgs = []
    for f in ("shard_start", "shard_len", "total", "flags", "entry", "exit_cut", "window_end",
              "first_cand_beyond"):
        if getattr(rec, f) != exp[f]:
            msgs.append(f"{f}: got {getattr(rec, f)}, oracle {exp[f]}")
    if rec.pad != 0:
        msgs.append(f"pad: got {rec.pad}, must be 0")
    for f, n in (("cands", rec.ncands), ("cuts", rec.ncuts)):
        if n > NCAP:
            msgs.append(f"n{f}: got {n} > {NCAP}")
            continue
        got = list(getattr(rec, f)[:n])
        d = _first_diff(got, exp[f], start, f)
        if n != len(exp[f]):
            msgs.append(f"n{f}: got {n}, oracle {len(exp[f])}")
        if d:
            msgs.append(d)
    return msgs


def check_record(rec, exp, start, note=""):
    msgs = mismatches(rec, exp, start)
    assert not msgs, f"record at start {start} {note}: " + "; ".join(msgs)


def _no_candidate_at_48(data, mn, av, mx):
    assert 48 not in o.candidates(data[:64], mn, av, mx).tolist()


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def uniform_1m():
    return o.synth_uniform(21, 0, 1 << 20)


@functools.lru_cache(maxsize=None)
def planted():
    """1 MiB of zeros with one 48-byte candidate block planted every 200 B
    from max + 100 to n - 4*max (48/256/8192, d = 192): from start 0 the chain
    makes a forced cut at max and then cuts at every plant."""
    mn, av, mx = SMALL
    d = o.discriminator(av)
    n = 1 << 20
    for seed in range(1, 100):
        rng = np.random.default_rng(seed)
        while True:
            blk = rng.integers(0, 256, 48, dtype=np.uint8)
            if o.window_hash(bytes(blk)) % d == d - 1:
                break
        alone = np.zeros(400, np.uint8)
        alone[176:224] = blk
        if o.candidates(alone, mn, av, mx).tolist() == [224]:
            break
    else:
        raise AssertionError("no block is a candidate on its own")
    data = np.zeros(n, np.uint8)
    for off in range(mx + 100, n - 4 * mx, 200):
        data[off:off + 48] = blk
    return data


@functools.lru_cache(maxsize=None)
def dense_tile():
    """test_periodic_dense_candidates' input: a candidate every 48 bytes."""
    P = o.params(*DEFAULT)
    rng = np.random.default_rng(1)
    while True:
        blk = rng.integers(0, 256, 48, dtype=np.uint8)
        if o.window_hash(bytes(blk)) % P.d == P.d - 1:
            break
    return np.tile(blk, (3 << 20) // 48)


@functools.lru_cache(maxsize=None)
def blob64():
    """The u64 blob of test_gpu_rotframe.py."""
    return o.synth_uniform(21, 0, (64 << 20) + 777)


@functools.lru_cache(maxsize=None)
def blob64_cands(prm):
    return o.candidates(blob64(), *prm)


# ---------------------------------------------------------------- 1. records
def _record_case(dctx, data, prm, shards, variant, pre):
    """`shards`: (start, length) pairs; `pre(start, exp)`: the case's condition
    on the oracle record, asserted before the first GPU call."""
    total = data.size
    exps = []
    for start, length in shards:
        if start == 0:
            _no_candidate_at_48(data, *prm)
        exp = expect(data, start, length, total, *prm)[0]
        pre(start, exp)
        exps.append(exp)
    t = torch_dev(data)
    p = _params(*prm)
    for (start, length), exp in zip(shards, exps):
        check_record(record(dctx, t, start, length, total, p, _flags(variant)), exp, start, variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_candidate_cap(dctx, variant):
    """1a: more than 1024 candidates in 32*max: window_end = cands[1023]."""
    data = uniform_1m()
    mx = SMALL[2]

    def pre(start, exp):
        assert len(exp["cands"]) == NCAP and exp["window_end"] < start + 32 * mx
        assert exp["window_end"] == exp["cands"][-1] and exp["first_cand_beyond"] != U64_MAX
        assert 700 < len(exp["cuts"]) < NCAP

    _record_case(dctx, data, SMALL, [(s, data.size - s) for s in (0, 4097, 53305)], variant, pre)


@pytest.mark.parametrize("variant", VARIANTS)
def test_cut_cap(dctx, variant):
    """1b: the 1024-cut cap ends the window before the 1024th candidate
    (start 0); from start 777 the same input comes out as the candidate cap."""
    data = planted()
    mx = SMALL[2]

    def pre(start, exp):
        c = o.candidates(data, *SMALL)
        c = c[c > start]
        if start == 0:
            assert len(exp["cuts"]) == NCAP and exp["cuts"][0] == mx
            assert exp["window_end"] == exp["cuts"][-1] < int(c[NCAP - 1])
            assert len(exp["cands"]) < NCAP and exp["first_cand_beyond"] == int(c[NCAP])
        else:
            # (no forced cut: all 1024 candidates are cuts, the cut cap is met but not passed)
            assert len(exp["cands"]) == NCAP and exp["cuts"] == exp["cands"]
            assert exp["window_end"] == exp["cands"][-1] == int(c[NCAP - 1])

    _record_case(dctx, data, SMALL, [(0, data.size), (777, data.size - 777)], variant, pre)


@pytest.mark.parametrize("variant", VARIANTS)
def test_short_last_window(dctx, variant):
    """1c: the last shard of a blob, shorter than 32*max: window_end == total."""
    from desync_amd import _lib

    def pre_for(prm, total):
        def pre(start, exp):
            assert total - start < 32 * prm[2]
            assert exp["flags"] == _lib.DSX_SEAM_LAST and exp["window_end"] == total
            assert len(exp["cands"]) < NCAP and exp["first_cand_beyond"] == U64_MAX
            assert len(exp["cands"]) > 50 or total - start < 100
            assert exp["cuts"] and exp["cuts"][-1] == total == exp["exit_cut"]
        return pre

    data = uniform_1m()
    n = data.size
    _record_case(dctx, data, SMALL, [(n - 150001, 150001), (n - 49, 49), (n - 1, 1)], variant,
                 pre_for(SMALL, n))
    data3 = o.synth_uniform(21, 0, (3 << 20) + 5)
    _record_case(dctx, data3, DEFAULT, [(0, data3.size), (12345, data3.size - 12345)], variant,
                 pre_for(DEFAULT, data3.size))


@pytest.mark.parametrize("variant", (HOST, DEVICE))
def test_empty_shard(dctx, variant):
    """1d: shard_len == 0 at the blob's end and inside it (the host-built
    record)."""
    data = uniform_1m()
    n = data.size

    def pre(start, exp):
        assert exp["cands"] == [] and exp["cuts"] == []
        assert exp["window_end"] == exp["exit_cut"] == exp["entry"] == start
        assert exp["flags"] == (oseam.SEAM_LAST if start == n else 0)

    _record_case(dctx, data, SMALL, [(n, 0), (4097, 0), (n - 1, 0)], variant, pre)


def test_dense_path_record(dctx):
    """1e: a candidate every 48 bytes: the scan's lane slots overflow, the
    shard is redone on the dense path and the record is built from the dense
    lists."""
    data = dense_tile()
    start = 48 * 1000 + 17
    exp = expect(data, start, data.size - start, data.size, *DEFAULT)[0]
    assert len(exp["cands"]) == NCAP and exp["cands"][0] == start + 31
    assert exp["window_end"] == start + 31 + 48 * (NCAP - 1) and 0 < len(exp["cuts"]) < NCAP
    t = torch_dev(data)
    before = dctx.stats().dense_fallbacks
    rec = record(dctx, t, start, data.size - start, data.size, _params(*DEFAULT), 0)
    assert dctx.stats().dense_fallbacks > before
    check_record(rec, exp, start, "dense")


@pytest.mark.parametrize("end", [9711770, 9711771, 9711822, 9711823])
def test_shard_end_off_the_word_grid(dctx, end):
    """A shard that ends inside the blob, 2 or 3 bytes past a 4-byte word
    boundary, with a candidate at its last or last but one position
    (9711822), or none where the window with those bytes read as zeros has
    one (9711770): the scan's buffer range used to end at the shard's last
    byte, and the dword across it read as zeros whole, so the chain's exit
    cut was 9711770 (not a cut) or missed 9711822.  The tiling below found it
    (48/256/8192, the shard from 8658874)."""
    data = blob64()[:10 << 20]
    total, start = data.size, 8658874
    exp = expect(data, start, end - start, total, *SMALL)[0]
    zeroed = data[:end].copy()
    zeroed[end - end % 4:] = 0
    true = o.candidates(data[:end], *SMALL)
    assert end % 4 >= 2 and true.tolist() != o.candidates(zeroed, *SMALL).tolist()
    assert exp["exit_cut"] == (9711822 if end >= 9711822 else 9711675)
    t = torch_dev(data)
    rec = record(dctx, t, start, end - start, total, _params(*SMALL), 0)
    check_record(rec, exp, start)
    # the candidates up to the shard's end, from a shard whose window holds them
    s2 = end - 100000
    exp2 = expect(data, s2, end - s2, total, *SMALL)[0]
    assert exp2["window_end"] == end and exp2["cands"][-1] == int(true[-1])
    check_record(record(dctx, t, s2, end - s2, total, _params(*SMALL), 0), exp2, s2)


def _tail_matters(data, start, end, prm):
    """The shard [start, end) ends inside the blob, and its candidates change
    when its last (end - start) % 4 bytes read as zeros (scan_kernel's loads
    are whole dwords from the piece's first byte)."""
    k = (end - start) % 4
    zeroed = data[:end].copy()
    zeroed[end - k:] = 0
    assert k and end < data.size
    assert o.candidates(data[:end], *prm).tolist() != o.candidates(zeroed, *prm).tolist()


@pytest.mark.parametrize("length", [40001, 40002, 40003, 39999])
def test_shard_end_off_the_word_grid_dense(dctx, length):
    """The same on the dense path (scan_kernel, which hashes the piece's last
    len % 4 positions again from byte loads): a candidate every 48 bytes, the
    shard ends inside the blob at a candidate (or, 39999, one byte past one)
    and its length is no multiple of 4.  The window holds the whole shard, so
    the record shows the last candidates."""
    data = dense_tile()
    end = 48 * 20000 + (1 if length == 39999 else 0)
    start = end - length
    _tail_matters(data, start, end, DEFAULT)
    exp = expect(data, start, length, data.size, *DEFAULT)[0]
    assert exp["window_end"] == end and exp["cands"][-1] == 48 * 20000 and exp["flags"] == 0
    t = torch_dev(data)
    before = dctx.stats().dense_fallbacks
    rec = record(dctx, t, start, length, data.size, _params(*DEFAULT), 0)
    assert dctx.stats().dense_fallbacks > before
    check_record(rec, exp, start, "dense")


@pytest.mark.parametrize("prm", [DEFAULT, SMALL])
def test_shard_end_off_the_word_grid_origin(dctx, prm):
    """The same where the blob starts off the 128-B line grid (data_ptr() +
    73, start 0: scan_kernel, no halo): shards [0, c) for the first
    candidates c of each residue c % 4 = 1, 2, 3, and [0, c + 1) with c % 4 =
    1, 2; the window holds the whole shard, so c must be its last candidate."""
    data = blob64()[:1 << 20]
    _no_candidate_at_48(data, *prm)
    cands = o.candidates(data, *prm)
    cands = cands[(cands > prm[0] + 100) & (cands < min(32 * prm[2], 100000 if prm == SMALL else 1 << 20))]
    ends = [int(cands[cands % 4 == r][0]) for r in (1, 2, 3)]
    ends += [int(cands[cands % 4 == r][0]) + 1 for r in (1, 2)]
    exps = []
    for end in ends:
        _tail_matters(data, 0, end, prm)
        exp = expect(data, 0, end, data.size, *prm)[0]
        assert exp["window_end"] == end and exp["cands"][-1] in (end, end - 1)
        assert len(exp["cands"]) < NCAP
        exps.append(exp)
    t = torch_dev(np.concatenate([np.zeros(73, np.uint8), data]))[73:]
    assert t.data_ptr() % 128 == 73
    for end, exp in zip(ends, exps):
        check_record(record(dctx, t, 0, end, data.size, _params(*prm), 0), exp, 0, f"end {end}")


# ---------------------------------------------------------------- 2. tiling
SHORT = (1 << 20) + 4321


def _tiling(prm, upto, whole):
    """The oracle records of the windows that tile blob64 up to `upto`: the
    first `whole` shards run from their start to the blob's end, the others
    are SHORT bytes long (several windows; at 48/256/8192 the stitch of a
    64 MiB shard takes a third of a second), the next one starts up to 127
    bytes before the record's window_end (a window that is not truncated
    ends 32*max after its start, which alone would keep every start on the
    first one's 128-B offset).  Returns (start, length, record, the record's
    candidates past the window before) per window."""
    data, cands = blob64(), blob64_cands(prm)
    total = data.size
    out, start, covered = [], 0, 0
    while covered < upto:
        length = total - start if len(out) < whole else min(total - start, SHORT)
        exp = expect(data, start, length, total, *prm, cands=cands)[0]
        assert exp["window_end"] > covered
        out.append((start, length, exp, [x for x in exp["cands"] if x > covered]))
        covered = exp["window_end"]
        start = covered - min((37 * len(out) + 5) % 128, covered - start - 1)
    return out


def _lanes():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 64


def _geometry(ptr, start, remaining, lanes):
    """(S, delta) of the line scan over the piece: lanes take a second
    384-byte trip once the grid exceeds 384 B per lane; the grid's origin is
    the 128-B line below the piece's first byte.  This restates
    enqueue_piece's choice (dsx_scan_geom.h) under the context's defaults: 8
    waves per workgroup (scanl_waves), one region per wave slot
    (regions_per_slot), no DSX_LANE_TARGET below 768, and every CU scanning.
    If one of those defaults changes, change `lanes` and this with it: the
    geometry cannot be read back from the product library."""
    delta = (ptr + start) & 127
    return (768 if remaining + delta > 384 * lanes else 384), delta


def _rotf_contexts(monkeypatch):
    from desync_amd import _lib
    ctxs = {}
    for rotf in ("1", "0"):
        monkeypatch.setenv("DSX_SCAN_ROTF", rotf)
        ctxs[rotf] = _lib.Context(0)
    monkeypatch.delenv("DSX_SCAN_ROTF")
    return ctxs


def _seam_bytes(rec):
    """The record's defined bytes: the header, cands[:ncands], cuts[:ncuts]
    (the entries past the counts are whatever the buffer held before)."""
    from desync_amd import _lib, shard
    b = shard.seam_to_bytes(rec)
    c0, k0 = _lib.Seam.cands.offset, _lib.Seam.cuts.offset
    return b[:c0] + b[c0:c0 + 8 * rec.ncands] + b[k0:k0 + 8 * rec.ncuts]


@pytest.mark.parametrize("name,prm,upto,off,whole", [
    ("default", DEFAULT, None, 0, 1 << 30),
    ("mid", MID, None, 0, 1 << 30),
    ("small", SMALL, 16 << 20, 0, 4),
    ("default+73", DEFAULT, None, 73, 1 << 30),
])
def test_tiling_every_candidate(monkeypatch, name, prm, upto, off, whole):
    """The windows' cands, concatenated, are o.candidates(blob) exactly, each
    record equals the oracle's, and the records of the two scan kernels
    (DSX_SCAN_ROTF=1 and =0) are the same bytes.  The first windows' pieces
    exceed 384 B per lane (S = 768, the trip-to-trip handoff), the later ones
    do not (S = 384); the starts put the grid origin at many offsets.  With
    off = 73 the blob itself starts off the line grid (scan_kernel at
    position 0).  At 48/256/8192 the windows tile the first 16 MiB, the
    first four from shards that run to the blob's end (S = 768), the others
    from shards of 1 MiB that end inside the blob: at that setting the stitch
    of a 64 MiB shard takes a third of a second, and 86 windows on two
    contexts took 57 s with every shard running to the end."""
    data = blob64()
    total = data.size
    cands = blob64_cands(prm)
    upto = total if upto is None else upto
    _no_candidate_at_48(data, *prm)
    tiles = _tiling(prm, upto, whole)
    want = cands[cands <= tiles[-1][2]["window_end"]]
    assert np.array_equal(np.array([x for *_, new in tiles for x in new], np.uint64), want)
    assert upto < total or want.size == cands.size
    # the fast path of expect (candidates computed once, C chain rule) is the
    # plain one: checked on the last, shortest windows
    for start, length, exp, _ in tiles[-2:]:
        assert expect(data, start, length, total, *prm)[0] == exp
    t = torch_dev(np.concatenate([np.zeros(off, np.uint8), data]))[off:]
    assert t.data_ptr() % 128 == off
    lanes = _lanes()
    geo = {_geometry(t.data_ptr(), s, n, lanes) for s, n, _, _ in tiles}
    assert len({d for _, d in geo}) >= 8, sorted(geo)
    assert {s for s, _ in geo} == {384, 768}, sorted(geo)
    p = _params(*prm)
    ctxs = _rotf_contexts(monkeypatch)
    try:
        for start, length, exp, _ in tiles:
            recs = {k: record(c, t, start, length, total, p, 0) for k, c in ctxs.items()}
            for k, rec in recs.items():
                check_record(rec, exp, start, f"{name} DSX_SCAN_ROTF={k}")
            assert _seam_bytes(recs["0"]) == _seam_bytes(recs["1"]), (name, start)
        # dsx_stats_t.candidates is reserved: the counts stay on the device
        assert [c.stats().candidates for c in ctxs.values()] == [0, 0]
    finally:
        for c in ctxs.values():
            c.close()


# ---------------------------------------------------------------- 3. protocol
def _zero_run(prm, seed=23):
    """_compose_shard("seam-zero-run") of test_gpu_parity.py scaled to prm: a
    zero run far longer than the 32*max window across the shard boundaries,
    entered off the max grid."""
    mx = prm[2]
    return np.concatenate([o.synth_uniform(seed + 1, 0, 3 * mx + 12345),
                           np.zeros(100 * mx, np.uint8), o.synth_uniform(seed, 0, 4 * mx)])


def equal_spans(total, world):
    span = total // world
    return [(r * span, span if r < world - 1 else total - r * span) for r in range(world)]


def geometry(bounds, total):
    """(start, length) per rank from the inner shard boundaries (a boundary
    given twice makes an empty shard)."""
    edges = [0] + list(bounds) + [total]
    return [(a, b - a) for a, b in zip(edges, edges[1:])]


def _oracle_protocol(data, world, prm, geo=None):
    """The protocol on the CPU: per round the records every rank publishes
    and oseam.resolve's outcome, then the final cuts per rank.  `geo`: the
    shards as (start, length), contiguous from 0 to data.size, lengths may be
    0; the default is `world` equal spans.  The last round's outcome is
    ("ok", [every rank's ext cuts])."""
    mn, av, mx = prm
    total = data.size
    geo = equal_spans(total, world) if geo is None else [(int(s), int(n)) for s, n in geo]
    assert len(geo) == world and geo[0][0] == 0 and sum(n for _, n in geo) == total
    assert all(n >= 0 and s + n == s2 for (s, n), (s2, _) in zip(geo, geo[1:]))
    loc = [expect(data, s, n, total, mn, av, mx) for s, n in geo]
    seams, spec, cands = [x[0] for x in loc], [x[1] for x in loc], [x[2] for x in loc]
    rounds = []
    while True:
        outs = [oseam.resolve(seams, r, mn, mx) for r in range(world)]
        ok = outs[0][0] == "ok"
        assert not ok or all(x[0] == "ok" for x in outs)
        rounds.append(([dict(s) for s in seams], ("ok", [list(x[1]) for x in outs]) if ok else outs[0]))
        if ok:
            # (seam_resolve_kernel's ext holds DSX_SEAM_MAX_CUTS cuts and no more)
            assert all(len(x[1]) < NCAP for x in outs)
            cuts = [oseam.rank_cuts(x[1], x[2], spec[r]) for r, x in enumerate(outs)]
            return geo, rounds, cuts
        assert all(x == outs[0] for x in outs) and len(rounds) <= world
        _, r, entry = outs[0]
        seams[r], spec[r] = oseam.rewalk(cands[r], entry, geo[r][0], geo[r][1], total, mn, mx)
        seams[r]["first_cand_beyond"] = U64_MAX


def _protocol(data, world, variant, prm, min_rounds=1, pre=None, geo=None, oracle=None, ctxs=None,
              t=None):
    """test_gpu_parity.py's _shard_protocol with the parameters and the shard
    geometry given (_oracle_protocol's `geo`), every round's records compared
    with oracle/seam.py's and every round's outcome with oseam.resolve's.

    variant: HOST (host records, dsx_shard_resolve), DEVICE (device records,
    dsx_shard_resolve) or ASYNC: dsx_shard_local with DSX_SEAM_DEVICE |
    DSX_NO_SYNC, then per round dsx_shard_resolve_async on every rank (device
    cuts, a device code word) and dsx_shard_collect on every rank; the code
    word must hold 0 after an ok round and 1 after a resync round, and the
    final cuts are read from the device buffers.

    oracle: _oracle_protocol's result, for a caller that has asserted its own
    conditions on it; ctxs: `world` contexts to use (and leave open); t: the
    blob on the device.  Returns (rounds, the cuts every rank got)."""
    import torch
    from desync_amd import _lib, shard
    assert variant in VARIANTS
    L = _lib.lib()
    total = data.size
    geo, rounds, want_cuts = oracle or _oracle_protocol(data, world, prm, geo)
    assert len(rounds) >= min_rounds
    assert np.array_equal(np.concatenate(want_cuts), o.chunk_stream(data, *prm))
    if pre:
        pre(rounds[0][0])
    t = torch_dev(data) if t is None else t
    p = _params(*prm)
    own = ctxs is None
    ctxs = [_lib.Context(0) for _ in range(world)] if own else list(ctxs[:world])
    assert len(ctxs) == world
    dev = variant != HOST
    try:
        if dev:
            recs = [torch.empty(shard.SEAM_BYTES, dtype=torch.uint8, device="cuda") for _ in range(world)]
            ptr = [x.data_ptr() for x in recs]
        else:
            recs = [_lib.Seam() for _ in range(world)]
            ptr = [ctypes.addressof(x) for x in recs]
        sflag = _lib.DSX_SEAM_DEVICE if dev else 0
        for r, (start, length) in enumerate(geo):
            _lib.check(L.dsx_shard_local(ctxs[r].h, ctypes.c_void_p(t.data_ptr() + start),
                                         64 if start else 0, start, length, total, ctypes.byref(p.c),
                                         ctypes.c_void_p(ptr[r]), _flags(variant)), ctxs[r].h)
        caps = [length // prm[0] + 4 + NCAP for _, length in geo]
        counts = [ctypes.c_uint64() for _ in range(world)]
        if variant == ASYNC:
            for c in ctxs:
                _lib.check(L.dsx_sync(c.h), c.h)
            outs = [torch.full((cap,), -1, dtype=torch.int64, device="cuda") for cap in caps]
            codes = [torch.full((1,), 0x5A5A, dtype=torch.int32, device="cuda") for _ in range(world)]
            agreed = ctypes.c_int32()
        else:
            outs = [np.empty(cap, np.uint64) for cap in caps]
        pieces = [c.stats().pieces for c in ctxs]
        for i, (seams, outcome) in enumerate(rounds):
            for r in range(world):
                rec = _read_back(ctxs[r], recs[r]) if dev else recs[r]
                check_record(rec, seams[r], geo[r][0], f"round {i + 1} rank {r}")
            if dev:
                allrec = torch.cat(recs)
                torch.cuda.synchronize()
                aptr = allrec.data_ptr()
            else:
                allrec = (_lib.Seam * world)(*recs)
                aptr = ctypes.addressof(allrec)
            if variant == ASYNC:
                for r in range(world):
                    codes[r].fill_(0x5A5A)
                torch.cuda.synchronize()
                for r in range(world):
                    _lib.check(L.dsx_shard_resolve_async(
                        ctxs[r].h, ctypes.c_void_p(aptr), world, r, ctypes.c_void_p(outs[r].data_ptr()),
                        caps[r], ctypes.c_void_p(codes[r].data_ptr())), ctxs[r].h)
                rcs = [L.dsx_shard_collect(ctxs[r].h, ctypes.c_void_p(ptr[r]), None, ctypes.byref(agreed),
                                           ctypes.byref(counts[r])) for r in range(world)]
                words = [int(c.item()) for c in codes]
                assert words == [0 if outcome[0] == "ok" else 1] * world, (i + 1, words, outcome)
            else:
                rcs = [L.dsx_shard_resolve(ctxs[r].h, ctypes.c_void_p(aptr), world, r,
                                           ctypes.c_void_p(ptr[r]), outs[r].ctypes.data, outs[r].size,
                                           ctypes.byref(counts[r]), sflag) for r in range(world)]
            # (the rank and entry of oseam.resolve's ("resync", rank, entry) are
            # checked through the next round's records: only that rank's record is
            # rewritten, with DSX_SEAM_REWALKED and that entry)
            want_rc = 0 if outcome[0] == "ok" else _lib.DSX_E_RESYNC
            assert rcs == [want_rc] * world, (i + 1, rcs, outcome)
        got_cuts = []
        for r in range(world):
            n = counts[r].value
            assert n <= caps[r], (r, n, caps[r])
            got = outs[r][:n].cpu().numpy().astype(np.uint64) if variant == ASYNC else outs[r][:n].copy()
            assert np.array_equal(got, want_cuts[r]), (r, _first_diff(got.tolist(), want_cuts[r].tolist(),
                                                                     geo[r][0], "cuts"))
            got_cuts.append(got)
        # a re-walk re-runs only the stitch over the kept candidate lists
        assert [c.stats().pieces for c in ctxs] == pieces
    finally:
        if own:
            for c in ctxs:
                c.close()
    return len(rounds), got_cuts


@pytest.mark.parametrize("world,dev", [(3, False), (4, True)])
def test_protocol_candidate_capped_windows(world, dev):
    data = o.synth_uniform(21, 0, (3 << 20) + 1001)
    _no_candidate_at_48(data, *SMALL)

    def pre(seams):
        for s in seams[1:]:
            assert len(s["cands"]) == NCAP and s["window_end"] == s["cands"][-1]

    _protocol(data, world, DEVICE if dev else HOST, SMALL, pre=pre)


def test_protocol_planted_cut_cap():
    data = planted()
    _no_candidate_at_48(data, *SMALL)

    def pre(seams):
        assert seams[1]["shard_start"] % 200 not in (0, (SMALL[2] + 100) % 200)
        assert len(seams[0]["cuts"]) == NCAP and seams[0]["window_end"] == seams[0]["cuts"][-1]

    _protocol(data, 2, HOST, SMALL, pre=pre)


@pytest.mark.parametrize("world,dev", [(2, False), (4, True)])
def test_protocol_zero_run_rewalks(world, dev):
    """Seams inside a zero run of 100*max do not converge in 32*max: the
    owners re-walk (DSX_E_RESYNC), and each rewritten record is
    oseam.rewalk's: DSX_SEAM_REWALKED, entry, exit_cut, empty lists."""
    data = _zero_run(MID)
    _no_candidate_at_48(data, *MID)
    assert _protocol(data, world, DEVICE if dev else HOST, MID, min_rounds=2)[0] > 1
