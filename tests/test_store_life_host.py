"""The life-cycle scripts on the model alone (store_life_ref.py): every
committed (profile, seed) script must contain the rare sequences the GPU test
exists for, the generator must be deterministic, and the driver's comparison
must notice a store that is wrong: three deliberately broken models are each
caught by every narrow script, at the first op they affect.  The known op
(dsx_chunk_ids_known) must come where the store has just lived: after a
compaction, a copy, a Grow, and on B straight after A."""
import numpy as np
import pytest

import store_copy_ref
import store_life_ref as life_ref
import store_prune_ref
import store_ref
from store_life_ref import Life, ModelBackend, Mismatch, conditions, drive, script

NARROW = [("narrow", s) for s in life_ref.NARROW_SEEDS]


def canon(v):
    """An op with its arrays as bytes, so that two ops compare with ==."""
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, (list, tuple)):
        return tuple(canon(x) for x in v)
    if isinstance(v, dict):
        return tuple((k, canon(x)) for k, x in sorted(v.items()))
    return v


def test_the_pool():
    pool = life_ref.pool_of("narrow")
    sizes = pool.sizes.tolist()
    assert len(sizes) == 900 and sizes.count(70000) == 3 and sizes.count(4097) == 9 and sizes.count(0) >= 10
    assert all(z == i % 50 for i, z in enumerate(sizes) if z not in (4097, 70000))
    assert 70000 > 65536  # longer than one gather tile
    for i in (0, 1, 96, 150, 899):
        want = life_ref._sum(pool.data(i))
        assert (pool.ids[i].tobytes() == want) == (i % 211 != 5)
    assert len(pool.liars) == 5
    wide = life_ref.pool_of("wide")
    assert len(wide.ids) == 140000 and int(wide.sizes.max()) == 15 and int(wide.sizes.min()) == 0
    # gather: the chunks back to back behind the pad, whatever the order
    blob, ids, ends, start = pool.gather([150, 3, 3, 0, 97], 7)
    assert start == 7 and ends.tolist() == [70007, 70010, 70013, 70013, 70060]
    assert blob[7:70007].tobytes() == pool.data(150) and blob[70013:70060].tobytes() == pool.data(97)
    assert np.array_equal(ids[1], pool.ids[3])


@pytest.mark.parametrize("profile,seed", NARROW)
def test_script_is_deterministic(profile, seed):
    a = script(profile, seed)
    life_ref._build.cache_clear()
    b = script(profile, seed)
    assert len(a) == len(b) == life_ref.PROFILES[profile]["ops"]
    assert a is not b and [canon(x) for x in a] == [canon(x) for x in b]


@pytest.mark.parametrize("profile,seed", NARROW)
def test_narrow_conditions(profile, seed):
    c = conditions(profile, seed)
    assert c["ops"] == 120
    assert c["put_after_prune"] >= 6, c
    assert c["prune_moves"] >= 10, c
    assert c["emptied"] >= 1 and c["put_after_emptied"] >= 1, c
    assert c["prune_3_windows"] >= 1, c
    assert c["put_refused"] >= 5, c
    assert c["copy_refused_missing"] >= 1, c
    assert c["copy_refused_capacity"] >= 1, c
    assert c["put_after_refusal"] >= 1, c
    assert c["copy_after_prune"] >= 1, c
    assert c["prune_after_copy"] >= 1, c
    assert c["grow"] >= 1 and c["grow_refused"] >= 1 and c["put_sealed"] >= 1, c
    assert c["up"] == [64, 256, 512] and c["down"] == [64, 256, 512], c
    # every kind of op, query and foreign call occurs
    assert set(c["kinds"]) == set(life_ref.MUTATING + life_ref.QUERIES + life_ref.FOREIGN), set(c["kinds"])
    ops = script(profile, seed)
    assert {op["store"] for op in ops if "store" in op} == {"A", "B", "C"}
    assert {op["ctx"] for op in ops if "ctx" in op} == {0, 1}
    for key in ("ids_dev", "ends_dev"):
        assert {op[key] for op in ops if op["op"] == "put"} == {True, False}
    for key, both in (("remove", {True, False}), ("window", {0, 65536}), ("ids_dev", {True, False})):
        assert {op[key] for op in ops if op["op"] == "prune"} == both, key
    assert any(op["op"] == "copy" and op["ids"] is None for op in ops)
    assert any(op["op"] == "copy" and op["ids"] is not None for op in ops)


def test_liars_share_no_bytes():
    """A known op recognises a liar's bytes under the liar's ID, so no other
    pool chunk may have those bytes (Pool.__init__ asserts it over all pairs;
    here by size: a liar shares its size with 17 others at the most, all
    random, and none is empty)."""
    pool = life_ref.pool_of("narrow")
    liars = [i for i in range(900) if i % 211 == 5]
    assert len(liars) == 5 and {pool.ids[i].tobytes() for i in liars} == pool.liars
    for i in liars:
        assert pool.sizes[i] >= 5
        assert all(pool.data(j) != pool.data(i) for j in range(900) if j != i)


@pytest.mark.parametrize("profile,seed", NARROW)
def test_known_conditions(profile, seed):
    """dsx_chunk_ids_known inside the store's life: right after an in-place
    compaction, a copy and a Grow of its store, on B straight after A (the two
    share a context's KnownScratch), with a liar's bytes recognised under the
    liar's ID, and chunks of every kind on either path."""
    c = life_ref.known_conditions(profile, seed)
    assert c["known"] >= 4, c
    assert c["after_prune_remove"] >= 1 and c["after_copy"] >= 1 and c["after_grow"] >= 1, c
    assert c["b_after_a"] >= 1, c
    assert c["liar_ids"] >= 3, c
    assert c["recognised"] >= 300 and c["hashed"] >= 300 and c["both_in_one"] >= 4, c
    assert c["big_recognised"] >= 1 and c["big_hashed"] >= 1 and c["empty_recognised"] >= 1, c
    # the periodic queries run it on every store, and never on the wide pool
    extras = [op for _, op, _, _, extra in life_ref.walk(profile, seed) if extra and op["op"] == "known"]
    assert len(extras) == 12 * 3 and {op["store"] for op in extras} == {"A", "B", "C"}
    assert all(op["pad"] % 2 == 1 for op in script(profile, seed) if op["op"] == "known")
    assert "known" in life_ref.QUERIES
    assert not any(op["op"] == "known" for _, op, _, _, _ in life_ref.walk("wide", 0))


def test_known_model_answers_by_bytes_then_by_id():
    """The op on a store with a liar: the chunk with the liar's bytes carries
    the liar's ID and its offset; a chunk the store lacks its hash and
    OFF_NONE; an empty chunk is recognised once the store holds one."""
    life = Life("narrow")
    pool = life.pool
    life.apply(life_ref._put_op("A", [7, 5, 0, 9], 3))
    res = life.apply(life_ref._known_op("A", [9, 5, 50, 11, 5, 7], 1))
    ids = [res["ids"][k:k + 32] for k in range(0, 192, 32)]
    assert ids[1] == ids[4] == pool.ids[5].tobytes() != life_ref._sum(pool.data(5))
    assert ids[1] in pool.liars
    assert ids[0] == life_ref._sum(pool.data(9)) and ids[3] == life_ref._sum(pool.data(11))
    assert ids[2] == life_ref._sum(b"") == pool.ids[0].tobytes()  # chunk 50 is empty as chunk 0 is
    assert res["known_off"] == [7 + 5, 7, 7 + 5, life_ref.store_ref.OFF_NONE, 7, 0]
    assert (res["recognised"], res["hashed"]) == (5, 1)


def test_wide_conditions():
    c = conditions("wide", 0)
    ops = script("wide", 0)
    assert [op["op"] for op in ops] == ["put", "prune", "put", "copy", "prune", "copy", "copy", "read"]
    # each of the three appends or keeps more than 65,536 entries in one call (the
    # scan's second pass then carries sums), right after a call of another kind
    assert c["put_over_65536"] >= 1 and c["prune_over_65536"] >= 2 and c["copy_over_65536"] >= 1, c
    assert c["copy_refused_capacity"] == 1 and c["copy_refused_missing"] == 1
    res = [step[2] for step in life_ref.walk("wide", 0)]
    assert len(res) == len(ops) == life_ref.PROFILES["wide"]["ops"]
    assert res[0]["totals"]["stored"] == 100000
    assert res[1]["totals"]["kept"] == 66666 and ops[1]["remove"] and ops[1]["ids_dev"]
    assert (res[2]["totals"]["stored"], res[2]["totals"]["present"]) == (40000, 30000)
    assert res[3]["refused"] == "capacity" and res[3]["totals"]["copied"] == 106666
    assert res[4]["totals"]["kept"] == 90000
    assert res[5]["refused"] is None and res[5]["totals"]["copied"] == 90000
    assert res[6]["refused"] == "missing" and res[6]["totals"]["missing"] == 2
    assert len(ops[7]["chunks"]) == 70002 and ops[7]["store"] == "B"
    t = res[7]["totals"]
    assert t["missing"] == t["wrong_size"] == t["beyond"] == 0 and t["pieces"] > 70000


# ---- the driver must be able to fail ----------------------------------------------------------
class NoRenumber(store_prune_ref.Store):
    """A prune that leaves the ID -> entry map with the numbers from before."""

    def prune(self, ids, remove=False):
        old = dict(self.pos)
        tot = super().prune(ids, remove)
        self.pos = {cid: old[cid] for cid in self.ids}
        return tot

    def locate(self, ids):
        offs, sizes, miss = [], [], 0
        for row in np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32):
            e = self.pos.get(row.tobytes())
            if e is None or e >= len(self.ends):
                offs.append(store_ref.OFF_NONE), sizes.append(0)
                miss += 1
            else:
                lo = self.ends[e - 1] if e else 0
                offs.append(lo), sizes.append(self.ends[e] - lo)
        return offs, sizes, miss

    def get(self, cid):
        e = min(self.pos[bytes(cid)], len(self.ends) - 1)
        return bytes(self.arena[(self.ends[e - 1] if e else 0):self.ends[e]])


class RefusedPutAdvances(store_prune_ref.Store):
    """A refused put that still adds its chunks to the count."""
    ghost = 0

    def put(self, blob, ids, ends, start=0):
        try:
            return super().put(blob, ids, ends, start)
        except store_ref.Capacity as e:
            self.ghost += e.totals["stored"]
            raise

    def counts(self):
        c = super().counts()
        c["chunks"] += self.ghost
        return c


def copy_in_id_order(dst, src, ids=None):
    """store_copy_ref.copy that appends the new chunks sorted by ID."""
    probe = store_prune_ref.Store(dst.arena_bytes, dst.max_chunks)
    probe.ids, probe.ends, probe.arena, probe.pos = list(dst.ids), list(dst.ends), bytearray(dst.arena), dict(dst.pos)
    totals = store_copy_ref.copy(probe, src, ids)
    new = sorted(probe.ids[len(dst.ids):])
    for cid in new:
        dst.pos[cid] = len(dst.ids)
        dst.ids.append(cid)
        dst.arena += src.get(cid)
        dst.ends.append(len(dst.arena))
    return totals


def first_affected(profile, seed, mutation):
    """Where each mutation first shows, worked out from the true model's walk
    alone: the first prune after which a survivor has another number; the first
    put refused for capacity; the first copy (a Grow is one) that appends IDs
    that are not in ascending order."""
    life = Life(profile)
    for pos, op in enumerate(script(profile, seed)):
        name = op.get("store")
        before = list(life.stores[name].ids) if name else []
        res = life.apply(op)
        after = life.stores[name].ids if name else []
        if mutation == "no_renumber" and op["op"] in ("prune", "remove_chunk"):
            if after != before[:len(after)]:
                return pos
        if mutation == "refused_put_advances" and op["op"] in ("put", "put_sealed"):
            if res["refused"] == "capacity":
                return pos
        if mutation == "copy_in_id_order" and op["op"] in ("copy", "grow") and not res["refused"]:
            new = after[len(before):] if op["op"] == "copy" else after
            if new != sorted(new):
                return pos
    raise AssertionError("the script never reaches the mutation")


MUTATIONS = {
    "no_renumber": lambda p: Life(p, store_cls=NoRenumber),
    "refused_put_advances": lambda p: Life(p, store_cls=RefusedPutAdvances),
    "copy_in_id_order": lambda p: Life(p, copy_fn=copy_in_id_order),
}


@pytest.mark.parametrize("profile,seed", NARROW)
def test_true_model_passes_the_driver(profile, seed):
    log = []
    drive(profile, seed, ModelBackend(Life(profile)), log=log)
    assert len(log) > 120 + 12 * 3 * len(life_ref.QUERIES)  # the placed ops, the states, the periodic queries
    assert sum(x[3] for x in log) == 12 * 3 * len(life_ref.QUERIES)
    own = []
    drive(profile, seed, ModelBackend(Life(profile)), log=own, extras=False)
    assert own == [x for x in log if not x[3]] and len(own) > 120


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
@pytest.mark.parametrize("profile,seed", NARROW)
def test_driver_detects_a_mutated_store(profile, seed, mutation):
    want = first_affected(profile, seed, mutation)
    with pytest.raises(Mismatch) as e:
        drive(profile, seed, ModelBackend(MUTATIONS[mutation](profile)))
    assert e.value.pos == want, str(e.value)
    text = str(e.value)
    assert f"{profile} seed {seed}, op {want}:" in text and "last five ops:" in text
    assert f"[{want}] " + life_ref.describe(script(profile, seed)[want]) in text


def test_wide_passes_the_driver():
    drive("wide", 0, ModelBackend(Life("wide")))
