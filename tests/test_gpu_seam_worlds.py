"""The shard seam protocol at 5 to 8 ranks, with short, tiny and empty shards.

tests/test_gpu_seam_record.py and test_gpu_parity.py run the protocol with at
most 4 ranks over equal spans, each many times `max`.  Here, in one process
with one context per simulated rank:

* re-walk cascades of world - 2 rounds (a zero run across every seam);
* non-final shards shorter than their 32*max window, than max, than min, of
  1, 48 and 49 bytes: such a shard may hold no cut, its record says exit_cut
  == shard_start, its seam cannot converge, and after its re-walk exit_cut is
  its entry, which the next rank's entry passes through;
* empty shards between non-empty ones, and a context that held a longer
  shard before it is given an empty one;
* a rank 0 without a cut;
* chunks that span three and more shards, and their IDs, whose prefix
  shard.rank_chunk_ids assembles from the tails of several earlier ranks;
* dsx_shard_resolve_async / dsx_shard_collect through re-walk rounds.

Every case states its point as a condition on oracle/seam.py's protocol,
asserted before the first GPU call of the case: a change of seed or geometry
that loses the point fails there.  The protocol itself is
test_gpu_seam_record._protocol: every round's records field by field, every
round's return codes, the final cuts per rank.
"""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from oracle import oracle as o
from test_gpu_seam_record import (ASYNC, DEVICE, HOST, MID, NCAP, SMALL, _no_candidate_at_48,
                                  _oracle_protocol, _params, _protocol, _zero_run, equal_spans,
                                  geometry, torch_dev)

pytestmark = pytest.mark.gpu

WORLD = 8


@pytest.fixture(scope="module")
def ranks():
    """One context per simulated rank, shared by the module's tests: a
    context is made for many calls, and one that is given a short or empty
    shard after a long one must not show the long one's state."""
    from desync_amd import _lib
    ctxs = [_lib.Context(0) for _ in range(WORLD)]
    yield ctxs
    for c in ctxs:
        c.close()


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def Z():
    return _zero_run(MID)


@functools.lru_cache(maxsize=None)
def R():
    return o.synth_uniform(21, 0, (1 << 20) + 1001)


@functools.lru_cache(maxsize=None)
def R3():
    return o.synth_uniform(21, 0, (3 << 20) + 1001)


Z0 = 3 * MID[2] + 12345  # the first zero of Z


@functools.lru_cache(maxsize=None)
def _on_device(name):
    return torch_dev({"Z": Z, "R": R, "R3": R3}[name]())


def _first_cuts():
    return [int(x) for x in o.chunk_stream(R(), *MID)[:3]]


def _bounds(case):
    mx = MID[2]
    if case == "short-in-zeros":
        return [40000, Z0 + 3000, Z0 + 8000, Z0 + 13000, Z0 + 18000, Z0 + 18000, Z0 + 18000 + 40 * mx]
    c0, c1, c2 = _first_cuts()
    if case == "tiny-round-cuts":
        return [c1 - 1, c1, c1 + 1, c1 + 49, c2 - 500, c2 - 500, c2 + 300]
    if case == "rank0-no-cut":
        return [100, 1000, c0, c0 + 1, c1 + 5]
    raise KeyError(case)


GEO_DATA = {"short-in-zeros": "Z", "tiny-round-cuts": "R", "rank0-no-cut": "R"}


@functools.lru_cache(maxsize=None)
def _oracle(name, prm, world, case=None):
    """_oracle_protocol of the input `name`, over equal spans or the
    boundaries of `case`; computed once, read by every variant."""
    data = {"Z": Z, "R": R, "R3": R3}[name]()
    _no_candidate_at_48(data, *prm)
    geo = equal_spans(data.size, world) if case is None else geometry(_bounds(case), data.size)
    assert len(geo) == world
    # dsx_shard_local reads a 64-byte halo in front of a shard
    assert all(s == 0 or s >= 64 for s, _ in geo)
    return _oracle_protocol(data, world, prm, geo)


def _rewalked(rounds):
    return [out[1] for _, out in rounds[:-1]]


def _no_cut_ranks(geo, cuts):
    return [r for r, (_, n) in enumerate(geo) if n and cuts[r].size == 0]


def _seams_in_a_chunk(data, prm, geo):
    """The most shard boundaries (one per seam, so an empty shard's two
    coincide and count twice) strictly inside one sequential chunk: such a
    chunk spans that many + 1 ranks."""
    ends = o.chunk_stream(data, *prm).tolist()
    seams = [s for s, _ in geo[1:]]
    return max(sum(a < b < e for b in seams) for a, e in zip([0] + ends, ends))


# ---------------------------------------------------------------- the cases
def pre_zero_run(world):
    geo, rounds, cuts = orc = _oracle("Z", MID, world)
    assert len(rounds) == world - 1
    assert _rewalked(rounds) == list(range(1, world - 1))
    assert all(n < 32 * MID[2] for _, n in geo)
    return "Z", MID, world, orc


def pre_short_in_zeros():
    geo, rounds, cuts = orc = _oracle("Z", MID, WORLD, "short-in-zeros")
    assert len(rounds) >= 5
    assert len(_no_cut_ranks(geo, cuts)) >= 2
    empty = [r for r, (_, n) in enumerate(geo) if n == 0]
    assert empty == [5] and cuts[5].size == 0 and 5 not in _rewalked(rounds)
    assert _seams_in_a_chunk(Z(), MID, geo) >= 3
    return "Z", MID, WORLD, orc


def pre_tiny_round_cuts():
    geo, rounds, cuts = orc = _oracle("R", MID, WORLD, "tiny-round-cuts")
    c0, c1, c2 = _first_cuts()
    assert [n for _, n in geo[1:4]] == [1, 1, 48] and geo[5][1] == 0
    assert len(rounds) >= 4 and 5 not in _rewalked(rounds)
    assert cuts[1].tolist() == [c1]
    assert sum(c.size == 0 for c in cuts) >= 3
    assert _seams_in_a_chunk(R(), MID, geo) >= 4
    return "R", MID, WORLD, orc


def pre_rank0_no_cut():
    geo, rounds, cuts = orc = _oracle("R", MID, 6, "rank0-no-cut")
    c0, c1, c2 = _first_cuts()
    first = rounds[0][0][0]
    assert first["exit_cut"] == 0 and first["cuts"] == [] and cuts[0].size == 0
    assert len(rounds) >= 2
    assert cuts[2].tolist() == [c0]
    return "R", MID, 6, orc


def pre_capped(world):
    geo, rounds, cuts = orc = _oracle("R3", SMALL, world)
    assert all(len(s["cands"]) == NCAP for s in rounds[0][0][1:])
    assert len(rounds) == 1
    assert any(rounds[0][1][1])  # true cuts ahead of some rank's convergence point
    return "R3", SMALL, world, orc


CASES = {
    "zero-run-5": lambda: pre_zero_run(5),
    "zero-run-7": lambda: pre_zero_run(7),
    "zero-run-8": lambda: pre_zero_run(8),
    "short-in-zeros": pre_short_in_zeros,
    "tiny-round-cuts": pre_tiny_round_cuts,
    "rank0-no-cut": pre_rank0_no_cut,
    "capped-5": lambda: pre_capped(5),
    "capped-8": lambda: pre_capped(8),
}
WITH_ASYNC = ("zero-run-5", "zero-run-7", "zero-run-8", "short-in-zeros", "tiny-round-cuts")


def _run(ranks, case, variant):
    name, prm, world, orc = CASES[case]()
    data = {"Z": Z, "R": R, "R3": R3}[name]()
    return orc, _protocol(data, world, variant, prm, oracle=orc, ctxs=ranks, t=_on_device(name))[1]


@pytest.mark.parametrize("variant", (HOST, DEVICE))
@pytest.mark.parametrize("case", list(CASES))
def test_protocol(ranks, case, variant):
    _run(ranks, case, variant)


@pytest.mark.parametrize("case", WITH_ASYNC)
def test_protocol_async(ranks, case):
    """dsx_shard_local with DSX_NO_SYNC, then dsx_shard_resolve_async and
    dsx_shard_collect per round: the device code word says 0 or 1 on every
    rank, the re-walks happen in collect, the cuts land in device memory."""
    _run(ranks, case, ASYNC)


def test_empty_shard_after_a_full_one(ranks):
    """A context that chunked a shard and is then given an empty one
    resolves to no cut: the chain state and cut list of the earlier shard
    must not reach shard_emit_kernel (which reads the count of speculative
    cuts on the device)."""
    from desync_amd import _lib
    L = _lib.lib()
    data = R()
    total = data.size
    want = o.chunk_stream(data, *MID)
    assert want[-1] == total  # a stale list would hold a cut >= the empty shard's start
    t = _on_device("R")
    p = _params(*MID)
    a, b = ranks[0], ranks[1]
    recs = (_lib.Seam * 2)()

    def local(ctx, rec, start, length):
        _lib.check(L.dsx_shard_local(ctx.h, ctypes.c_void_p(t.data_ptr() + start), 64 if start else 0,
                                     start, length, total, ctypes.byref(p.c),
                                     ctypes.c_void_p(ctypes.addressof(rec)), 0), ctx.h)

    local(b, recs[1], 64, total - 64)
    assert recs[1].exit_cut == total
    local(a, recs[0], 0, total)
    local(b, recs[1], total, 0)
    out = np.empty(total // MID[0] + 4 + NCAP, np.uint64)
    n = ctypes.c_uint64(99)
    for ctx, r, exp in ((b, 1, []), (a, 0, want.tolist())):
        _lib.check(L.dsx_shard_resolve(ctx.h, ctypes.c_void_p(ctypes.addressof(recs)), 2, r,
                                       ctypes.c_void_p(ctypes.addressof(recs[r])), out.ctypes.data,
                                       out.size, ctypes.byref(n), 0), ctx.h)
        assert out[:n.value].tolist() == exp, (r, n.value)


# ---------------------------------------------------------------- chunk IDs
def _tails_want(geo, cuts):
    """(has_cut, length) of every rank's tail_record, and for every rank
    with a cut the number of tails its first chunk's prefix is made of."""
    heads = []
    for (s, n), c in zip(geo, cuts):
        heads.append((1, s + n - int(c[-1])) if c.size else (0, n))
    depth = {}
    for r, c in enumerate(cuts):
        if c.size:
            q = r - 1
            while q > 0 and not heads[q][0]:
                q -= 1
            depth[r] = r - max(q, 0)
    return heads, depth


@pytest.mark.parametrize("algo", ["sha512-256", "sha256"])
@pytest.mark.parametrize("case", list(GEO_DATA))
def test_chunk_ids_over_multi_shard_chunks(ranks, case, algo):
    """shard.tail_record and shard.rank_chunk_ids per rank, as
    shard_chunk_ids calls them between its all-gather: the prefix of a
    chunk that spans several shards comes from the tails of all the ranks
    back to the first one that has a cut, whole shards (has_cut == 0) and
    empty tails included."""
    from desync_amd import _lib, shard
    name, prm, world, orc = CASES[case]()
    geo, _, want_cuts = orc
    heads, depth = _tails_want(geo, want_cuts)
    assert any(h == 0 and n > 0 for h, n in heads)
    assert any(n == 0 for _, n in heads)
    # some rank's prefix is made of three tails or more; the six shards of
    # "rank0-no-cut" allow two, and there the point is that the walk back
    # reaches rank 0 without meeting a rank that has a cut
    if case == "rank0-no-cut":
        assert depth[2] == 2 and heads[0][0] == heads[1][0] == 0
    else:
        assert max(depth.values()) >= 3, depth
    data = {"Z": Z, "R": R, "R3": R3}[name]()
    raw = data.tobytes()
    hname = {"sha512-256": "sha512_256", "sha256": "sha256"}[algo]
    code = {"sha512-256": _lib.DSX_DIGEST_SHA512_256, "sha256": _lib.DSX_DIGEST_SHA256}[algo]
    _, cuts = _run(ranks, case, HOST)
    t = _on_device(name)
    ptr = [t.data_ptr() + s for s, _ in geo]
    tails = [shard.tail_record(ranks[r], ptr[r], geo[r][0], geo[r][1], cuts[r], prm[2])
             for r in range(world)]
    got_heads = [tuple(int(x) for x in np.frombuffer(x[:16], np.uint64)) for x in tails]
    assert got_heads == heads
    ends = o.chunk_stream(data, *prm).tolist()
    start_of = dict(zip(ends, [0] + ends))
    nids = 0
    for r in range(world):
        ids = shard.rank_chunk_ids(ranks[r], ptr[r], geo[r][0], geo[r][1], cuts[r], tails, r, code)
        want = [hashlib.new(hname, raw[start_of[e]:e]).digest() for e in cuts[r].tolist()]
        assert [bytes(i) for i in ids] == want, f"rank {r} of {geo}"
        nids += len(ids)
    assert nids == len(ends)
