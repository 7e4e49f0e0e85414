"""Use tracking and eviction of the chunk store, without a GPU: the ABI names,
the model (store_evict_ref.py) against brute force over all prefixes, the
bucket choice of the radix descent (dsx_evict_geom.h) under the host
sanitizers, and the life scripts against the planted-mistake models."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import store_evict_ref as ref
import store_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsx_store_track", "dsx_store_touch", "dsx_store_stamps", "dsx_store_evict")


def test_names():
    """The four calls are bound and declared, the totals are 104 bytes, the
    constants are the header's and the Python names exist."""
    import desync_amd
    from desync_amd import _lib
    with open(os.path.join(REPO, "include", "dsx.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert ctypes.sizeof(_lib.StoreEvictTotals) == 104
    assert re.search(r"#define DSX_EVICT_DRY (\d+)u", header).group(1) == str(_lib.DSX_EVICT_DRY)
    assert re.search(r"#define DSX_STAMP_NOW (\d+)ull", header).group(1) == str(_lib.DSX_STAMP_NOW)
    for flag in ("DSX_IDS_DEVICE", "DSX_PRUNE_REMOVE", "DSX_COPY_ALL", "DSX_OUT_DEVICE", "DSX_ENDS_DEVICE"):
        assert getattr(_lib, flag) != _lib.DSX_EVICT_DRY
    for name in ("Track", "Touch", "Evict", "stamps"):
        assert callable(getattr(desync_amd.DeviceStore, name))
    import inspect
    params = inspect.signature(desync_amd.DeviceStore.__init__).parameters
    assert params["track"].default is False and params["evict"].default is False


def _random_store(rng, n):
    s = ref.Store(1 << 20, 64, track=True)
    sizes = rng.integers(0, 4, n) * rng.integers(0, 50, n)
    ends = np.cumsum(sizes).astype(np.uint64)
    ids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s.put(bytes(rng.integers(0, 256, int(ends[-1]) + 1, dtype=np.uint8)), ids, ends)
    s.stamps = [int(t) for t in rng.integers(0, 4, n)]
    s.clock = 3
    return s, ids


@pytest.mark.parametrize("seed", range(40))
def test_model_against_brute_force(seed):
    """On small random stores: the victims are a prefix of the use order, no
    shorter prefix makes the room, and a need no prefix meets is refused with
    the store unchanged."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 12))
    s, ids = _random_store(rng, n)
    pin = ids[rng.random(n) < 0.3]
    pinned = {r.tobytes() for r in pin}
    order = sorted((e for e in range(n) if s.ids[e] not in pinned), key=lambda e: (s.stamps[e], e))
    used, room_c = len(s.arena), s.max_chunks - n
    for need_c, need_b in itertools.product((0, room_c, room_c + 1, room_c + n // 2, room_c + n + 1),
                                            (0, s.arena_bytes - used + 1, s.arena_bytes - used // 2, s.arena_bytes,
                                             s.arena_bytes + 1)):
        fits = [k for k in range(len(order) + 1)
                if s.arena_bytes - used + sum(s.size(e) for e in order[:k]) >= need_b
                and room_c + k >= need_c]
        t = ref.Store.__new__(ref.Store)
        t.__dict__ = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in s.__dict__.items()}
        if not fits:
            with pytest.raises(store_ref.Capacity) as exc:
                t.evict(need_b, need_c, pin)
            assert (t.ids, t.ends, t.arena, t.stamps) == (s.ids, s.ends, s.arena, s.stamps)
            assert exc.value.totals["evictable"] == len(order) and exc.value.totals["pinned"] == n - len(order)
            continue
        victims = sorted(order[:fits[0]])
        tot = t.evict(need_b, need_c, pin)
        assert tot["ids"] == b"".join(s.ids[e] for e in victims)
        assert tot["evicted"] == len(victims) and tot["kept"] == n - len(victims)
        assert tot["evicted_bytes"] == sum(s.size(e) for e in victims)
        assert tot["cutoff"] == max((s.stamps[e] for e in victims), default=0)
        keep = [e for e in range(n) if e not in victims]
        assert t.ids == [s.ids[e] for e in keep] and t.stamps == [s.stamps[e] for e in keep]
        assert bytes(t.arena) == b"".join(s.get(s.ids[e]) for e in keep)
        assert all(cid in t.pos for cid in pinned if cid in s.pos)


def test_evict_geom_model(tmp_path):
    """dsx_evict_geom.h alone, under the host sanitizers: the descent made of
    its bucket choice against a linear walk of the sorted entries over seeded
    histograms (tests/evict_geom_model.cpp); a difference is a non-zero exit."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "evict_geom_model")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(REPO, "desync_amd", "csrc"),
           os.path.join(REPO, "tests", "evict_geom_model.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1].startswith("evict geom model ok: "), r.stdout[-1000:]


class _ModelBackend:
    def __init__(self, cls):
        self.life = ref.Life(cls)

    def apply(self, op):
        return self.life.apply(op)

    def state(self, name):
        return self.life.state(name)


@pytest.mark.parametrize("seed", ref.LIFE_SEEDS)
def test_life_scripts(seed):
    """A script runs clean on the true model, holds every kind of call, evicts
    that removed and that were refused, and is told apart from every planted
    mistake."""
    ops = ref.script(seed)
    assert len(ops) >= ref.LIFE_OPS
    assert {"put", "copy", "touch", "evict", "prune", "grow"} <= {op["op"] for op in ops}
    ref.drive(seed, _ModelBackend(ref.Store))
    life, evicted, refused, carried = ref.Life(), 0, 0, 0
    for op in ops:
        empty = not life.stores[op["store"]].ids
        res = life.apply(op)
        if op["op"] == "evict":
            evicted += bool(not res["refused"] and res["totals"]["evicted"] and not op["dry"])
            refused += res["refused"] == "capacity"
        all_into_empty = op["op"] == "grow" or (op["op"] == "copy" and op["ids"] is None and empty)
        carried += all_into_empty and res["totals"]["copied"] > 0
    assert evicted >= 3 and carried >= 2, (evicted, refused, carried)
    for mutant in ref.MUTANTS:
        with pytest.raises(ref.Mismatch):
            ref.drive(seed, _ModelBackend(mutant))


def test_life_scripts_refuse():
    """Over the scripts an evict is refused for capacity at least once."""
    refused = 0
    for seed in ref.LIFE_SEEDS:
        life = ref.Life()
        for op in ref.script(seed):
            refused += life.apply(op).get("refused") == "capacity" and op["op"] == "evict"
    assert refused >= 1
