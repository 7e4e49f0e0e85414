"""dsx_plan_walk (SeedSequencer.Plan over 32-bit classes, host code): against
the brute-force restatement of the reference in seedplan_ref.py, on the
goldens, random ID strings, long equal runs, ABAB..., crafted arrays, and the
capacity and empty cases.  No GPU."""
import ctypes
import os
import random
import time

import numpy as np
import pytest

import seedplan_ref as ref
from desync_amd import _lib
from desync_amd.digest import NewNullChunk
from desync_amd.index import IndexFromReader

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIMITS = (0, 1, 2, 3, 5, 100)


def load_index(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return IndexFromReader(f)


def id_sizes(ix):
    return [bytes(c.ID) for c in ix.Chunks], [int(c.Size) for c in ix.Chunks]


def by_source(segs):
    return (sum(1 for g in segs if g[4] >= 0), sum(1 for g in segs if g[4] == ref.SRC_NULL),
            sum(1 for g in segs if g[4] == ref.SRC_STORE))


# ---- case 1: the goldens ----------------------------------------------------------
# (limit, null seed) -> (segments, from the file seed, null, store): the
# restatement's figures for blob2.caibx from seed blob1.caibx
GOLDEN_COUNTS = {(0, True): (12, 5, 0, 7), (0, False): (12, 5, 0, 7),
                 (100, True): (12, 5, 0, 7), (100, False): (12, 5, 0, 7),
                 (3, True): (60, 43, 10, 7)}


@pytest.mark.parametrize("null_seed", (True, False))
@pytest.mark.parametrize("limit", (0, 100, 3))
@pytest.mark.parametrize("target,seed", (("blob2.caibx", "blob1.caibx"), ("blob1.caibx", "blob2.caibx")))
def test_goldens(target, seed, limit, null_seed):
    tix, six = load_index(target), load_index(seed)
    ids, sizes = id_sizes(tix)
    assert ids.count(NewNullChunk(tix.Index.ChunkSizeMax).ID) == 31
    null_id = NewNullChunk(tix.Index.ChunkSizeMax).ID if null_seed else None
    want = ref.plan(ids, sizes, [id_sizes(six)], null_id, limit)
    got = ref.walk(ids, sizes, [id_sizes(six)], null_id, limit)
    assert got == want
    segs = got[0]
    assert sum(g[1] for g in segs) == len(ids) and sum(g[3] for g in segs) == tix.Length()
    counts = GOLDEN_COUNTS.get((limit, null_seed))
    if counts is not None:
        if target == "blob2.caibx":
            assert (len(segs),) + by_source(segs) == counts
        else:
            assert len(segs) == counts[0]


# ---- case 2: random ID strings ---------------------------------------------------
def random_case(rng):
    k = rng.randint(1, 4)
    alphabet = list(range(k))
    n = rng.randint(1, 60)
    ids = [rng.choice(alphabet) for _ in range(n)]
    sizes = [rng.randint(1, 4) for _ in range(n)]
    seeds = []
    for _ in range(rng.randint(1, 3)):
        m = rng.randint(1, 60)
        # now and then a copy of a stretch of the target, so long matches and
        # equal-byte ties between seeds occur
        if rng.random() < 0.4:
            a = rng.randrange(n)
            sids = ([rng.choice(alphabet) for _ in range(rng.randint(0, 5))] + ids[a:a + m])[:m] or [0]
        else:
            sids = [rng.choice(alphabet) for _ in range(m)]
        seeds.append((sids, [rng.randint(1, 4) for _ in sids]))
    null_id = rng.choice([None, 0, 0, k])  # k: a null ID no chunk has
    return ids, sizes, seeds, null_id, rng.choice([0, 0, 7])


@pytest.mark.parametrize("limit", LIMITS)
def test_random_id_strings(limit):
    rng = random.Random(1000 + limit)
    for _ in range(300):
        ids, sizes, seeds, null_id, start = random_case(rng)
        want = ref.plan(ids, sizes, seeds, null_id, limit, start)
        got = ref.walk(ids, sizes, seeds, null_id, limit, start)
        assert got == want, (ids, sizes, seeds, null_id, limit, start)


# ---- case 3: equal runs -----------------------------------------------------------
@pytest.mark.parametrize("limit", (0, 100))
@pytest.mark.parametrize("n", (70000, 300000))
def test_equal_runs(n, limit):
    """n equal IDs on both sides, no null seed: without the run shortcut the
    walk compares ~n^2 / 2 IDs (4.5e10 at 300,000)."""
    size = 3
    zeros = np.zeros(n, dtype=np.uint32)
    ends = ref.ends_of([size] * n)
    t0 = time.perf_counter()
    rc, segs, store, tot = ref.raw_walk(ends, 0, zeros, None, [(zeros, zeros, ends)], limit, n, n)
    dt = time.perf_counter() - t0
    print(f"dsx_plan_walk n={n} limit={limit}: {dt * 1e3:.1f} ms")
    assert rc == _lib.DSX_OK
    if limit == 0:
        assert segs == [(0, n, 0, size * n, 0, 0, 0)]
    else:
        want = [(i, min(limit, n - i), size * i, size * min(limit, n - i), 0, 0, 0)
                for i in range(0, n, limit)]
        assert len(want) == -(-n // limit) and segs == want
    assert store == [] and tot["seed_chunks"] == n and tot["seed_bytes"] == size * n
    assert dt < 5.0


# ---- case 4: ABAB... --------------------------------------------------------------
@pytest.mark.parametrize("limit", (0, 100))
def test_abab(limit):
    n = 2000
    ids = [i & 1 for i in range(n)]
    sizes = [1 + (i % 3) for i in range(n)]
    seeds = [([(i + 1) & 1 for i in range(n - 3)], [2] * (n - 3)), (ids[:700], [3] * 700)]
    assert ref.walk(ids, sizes, seeds, None, limit) == ref.plan(ids, sizes, seeds, None, limit)


# ---- case 5: crafted arrays ---------------------------------------------------------
def _good():
    """A well-formed call: target ABCA, seed BCAB."""
    ids, sids = [0, 1, 2, 0], [1, 2, 0, 1]
    t, s = ref.classes(ids, sids)
    return dict(ends=ref.ends_of([5, 6, 7, 5]), first=ref.first_positions(ids), t=t, s=s,
                sends=ref.ends_of([6, 7, 5, 6]), is_null=np.zeros(4, np.uint8))


def _call(a, limit=0):
    return ref.raw_walk(a["ends"], 0, a["first"], a["is_null"], [(a["t"], a["s"], a["sends"])],
                        limit, 16, 16)[0]


def test_crafted_baseline_is_accepted():
    assert _call(_good()) == _lib.DSX_OK


@pytest.mark.parametrize("what", ("sclass_above_p", "sclass_not_idempotent", "tclass_out_of_range",
                                  "tclass_huge", "tclass_not_fixed_point", "first_pos_above_i",
                                  "ends_decrease", "seed_ends_decrease", "ends_below_start"))
def test_crafted_arrays_are_refused(what):
    a = _good()
    start = 0
    if what == "sclass_above_p":
        a["s"][1] = 3
    elif what == "sclass_not_idempotent":
        a["s"][:] = [0, 0, 1, 0]  # class 1 is itself of class 0
    elif what == "tclass_out_of_range":
        a["t"][2] = 4
    elif what == "tclass_huge":
        a["t"][0] = 0xFFFFFFFE
    elif what == "tclass_not_fixed_point":
        a["t"][0] = 3  # sclass[3] == 0
    elif what == "first_pos_above_i":
        a["first"][1] = 2
    elif what == "ends_decrease":
        a["ends"][2] = a["ends"][1] - 1
    elif what == "seed_ends_decrease":
        a["sends"][3] = 1
    elif what == "ends_below_start":
        start = 6
    rc = ref.raw_walk(a["ends"], start, a["first"], a["is_null"], [(a["t"], a["s"], a["sends"])],
                      0, 16, 16)[0]
    assert rc == _lib.DSX_E_INVAL


def test_counts_above_the_limit_are_refused():
    tot = _lib.PlanTotals()
    L = _lib.lib()
    big = 0xFFFFFFF1
    one = np.zeros(1, np.uint64)
    assert L.dsx_plan_walk(ctypes.c_void_p(one.ctypes.data), 0, big, ctypes.c_void_p(one.ctypes.data),
                           None, None, 0, 0, None, 0, None, 0, ctypes.byref(tot)) == _lib.DSX_E_INVAL
    ps = (_lib.PlanSeed * 1)()
    ps[0].m = big
    assert L.dsx_plan_walk(ctypes.c_void_p(one.ctypes.data), 0, 0, None, None,
                           ctypes.cast(ps, ctypes.c_void_p), 1, 0, None, 0, None, 0,
                           ctypes.byref(tot)) == _lib.DSX_E_INVAL
    assert L.dsx_plan_walk(None, 0, 0, None, None, None, 0, 0, None, 0, None, 0, None) \
        == _lib.DSX_E_INVAL  # (no totals)


# ---- case 6: capacity ---------------------------------------------------------------
def test_capacity():
    ids = [0, 1, 9, 9, 1, 8, 9]
    sizes = [2, 3, 4, 4, 3, 5, 4]
    seeds = [([5, 0, 1, 6], [1, 2, 3, 1])]
    want = ref.plan(ids, sizes, seeds)
    assert want[2]["segments"] == 6 and want[2]["store_unique"] == 2 and want[1] == [2, 5]
    t, s = ref.classes(ids, seeds[0][0])
    args = (ref.ends_of(sizes), 0, ref.first_positions(ids), None, [(t, s, ref.ends_of(seeds[0][1]))], 0)
    for seg_cap, store_cap in ((0, 0), (5, 2), (6, 1), (3, 0)):
        rc, segs, store, tot = ref.raw_walk(*args, seg_cap, store_cap)
        assert rc == _lib.DSX_E_CAPACITY
        assert tot == want[2]  # the required counts, and every total
        assert segs == want[0][:seg_cap] and store == want[1][:store_cap]
    rc, segs, store, tot = ref.raw_walk(*args, 6, 2)
    assert rc == _lib.DSX_OK and (segs, store, tot) == want


# ---- case 7: n == 0 -----------------------------------------------------------------
def test_empty_target():
    e = np.zeros(0, np.uint64)
    z = np.zeros(0, np.uint32)
    s = np.zeros(3, np.uint32)
    rc, segs, store, tot = ref.raw_walk(e, 0, z, None, [(z, s, ref.ends_of([1, 1, 1]))], 0, 4, 4)
    assert rc == _lib.DSX_OK and segs == [] and store == [] and not any(tot.values())
    rc, segs, store, tot = ref.raw_walk(e, 0, z, None, [], 100, 0, 0)
    assert rc == _lib.DSX_OK and not any(tot.values())
    # an empty seed matches nothing
    assert ref.walk([1, 2], [3, 4], [([], [])]) == ref.plan([1, 2], [3, 4], [([], [])])


# ---- case 8: exports and the package ------------------------------------------------
def test_exports_and_layouts():
    L = _lib.lib()
    for name in ("dsx_plan_walk", "dsx_seed_plan", "dsx_assemble"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert ctypes.sizeof(_lib.PlanSeg) == 40
    assert [(n, getattr(_lib.PlanSeg, n).offset) for n, _ in _lib.PlanSeg._fields_] == [
        ("dst_off", 0), ("bytes", 8), ("src_off", 16), ("first", 24), ("count", 28),
        ("source", 32), ("seed_first", 36)]
    assert ctypes.sizeof(_lib.PlanTotals) == 9 * 8
    assert [n for n, _ in _lib.PlanTotals._fields_] == [
        "segments", "seed_chunks", "seed_bytes", "null_chunks", "null_bytes", "store_chunks",
        "store_bytes", "store_unique", "store_len"]
    assert ctypes.sizeof(_lib.PlanSeed) == 32
    assert (_lib.DSX_SRC_NULL, _lib.DSX_SRC_STORE) == (-1, -2)
    assert (_lib.DSX_STORE_DEVICE, _lib.DSX_ASSEMBLE_UNALIGNED, _lib.DSX_ASSEMBLE_TILE) == (128, 256, 65536)
    # the new flags collide with no flag they can be combined with
    others = (_lib.DSX_OUT_DEVICE, _lib.DSX_NO_SYNC, _lib.DSX_ENDS_DEVICE, _lib.DSX_SEAM_DEVICE,
              _lib.DSX_TIMED, _lib.DSX_IDS_DEVICE, _lib.DSX_SIZES)
    assert all(f & (_lib.DSX_STORE_DEVICE | _lib.DSX_ASSEMBLE_UNALIGNED) == 0 for f in others)
    assert L.dsx_abi_version() == 5


def test_package_exports_the_python_layer():
    import desync_amd
    for name in ("NewIndexSeed", "NewSeedSequencer", "SeedSequencer", "Plan", "AssembleBlob",
                 "SeedInvalid", "IndexSeed"):
        assert name in desync_amd.__all__ and hasattr(desync_amd, name), name
    assert hasattr(desync_amd.MemoryStore, "GetChunk")


def test_null_context_is_invalid():
    L = _lib.lib()
    tot = _lib.PlanTotals()
    assert L.dsx_seed_plan(None, None, None, 0, 0, None, None, None, 0, None, 0, None, 0, None, 0,
                           ctypes.byref(tot), 0) == _lib.DSX_E_INVAL
    assert L.dsx_assemble(None, None, 0, None, None, 0, None, 0, None, 0, 0) == _lib.DSX_E_INVAL


def test_plan_walk_builds_and_replays_without_hip(tmp_path):
    """dsx_plan.cpp includes nothing of HIP: a plain C++ compiler builds it with
    tests/plan_replay.cpp (the program meant for -fsanitize=address,undefined),
    and the replay agrees with that program's own brute force."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "plan_replay")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(repo, "include"),
                    os.path.join(repo, "tests", "plan_replay.cpp"),
                    os.path.join(repo, "desync_amd", "csrc", "dsx_plan.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)
