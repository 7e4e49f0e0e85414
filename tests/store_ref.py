"""A dict-and-bytearray model of the chunk store in HBM (dsx_store_*): the
first-occurrence order, the totals, the all-or-nothing capacity rule, locate
and resolve.  The GPU tests compare the arena, the entries and the totals with
it byte for byte."""
import numpy as np

OFF_NONE = 0xFFFFFFFFFFFFFFFF
SRC_STORE = -2


class Capacity(Exception):
    def __init__(self, totals):
        super().__init__("the put does not fit")
        self.totals = totals


class Store:
    def __init__(self, arena_bytes, max_chunks):
        self.arena_bytes, self.max_chunks = int(arena_bytes), int(max_chunks)
        self.arena = bytearray()
        self.ids = []    # entry -> ID
        self.ends = []   # entry -> cumulative end
        self.pos = {}    # ID -> entry

    def counts(self):
        return {"chunks": len(self.ids), "bytes": len(self.arena), "max_chunks": self.max_chunks,
                "arena_bytes": self.arena_bytes}

    def put(self, blob, ids, ends, start=0):
        """-> totals; raises Capacity (with the would-be totals) and changes
        nothing if the new chunks do not fit."""
        blob = memoryview(bytes(blob) if not isinstance(blob, (bytes, bytearray, memoryview)) else blob)
        ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)
        ends = [int(e) for e in ends]
        n = len(ends)
        assert n == len(ids)
        prev = int(start)
        for e in ends:
            assert prev <= e <= len(blob), "a malformed chunk list is refused before the model"
            prev = e
        seen, new = set(), []
        present = 0
        prev = int(start)
        for i in range(n):
            cid = ids[i].tobytes()
            lo, prev = prev, ends[i]
            if cid in seen:
                continue
            seen.add(cid)
            if cid in self.pos:
                present += 1
            else:
                new.append((cid, lo, ends[i]))
        stored_bytes = sum(hi - lo for _, lo, hi in new)
        totals = {"total": n, "stored": len(new), "stored_bytes": stored_bytes, "present": present,
                  "repeats": n - len(new) - present}
        if len(self.ids) + len(new) > self.max_chunks or len(self.arena) + stored_bytes > self.arena_bytes:
            raise Capacity(totals)
        for cid, lo, hi in new:
            self.pos[cid] = len(self.ids)
            self.ids.append(cid)
            self.arena += blob[lo:hi]
            self.ends.append(len(self.arena))
        return totals

    def entries(self):
        ids = np.frombuffer(b"".join(self.ids), dtype=np.uint8).reshape(-1, 32)
        return ids, np.array(self.ends, dtype=np.uint64)

    def locate(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)
        offs, sizes, miss = [], [], 0
        for row in ids:
            e = self.pos.get(row.tobytes())
            if e is None:
                offs.append(OFF_NONE), sizes.append(0)
                miss += 1
            else:
                lo = self.ends[e - 1] if e else 0
                offs.append(lo), sizes.append(self.ends[e] - lo)
        return offs, sizes, miss

    def get(self, cid):
        e = self.pos[bytes(cid)]
        return bytes(self.arena[(self.ends[e - 1] if e else 0):self.ends[e]])

    def resolve(self, ids, segs):
        """dsx_store_resolve on a structured segment array -> (n_missing,
        n_wrong_size, first_bad); rewrites src_off only if both are zero."""
        ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)
        miss = wrong = 0
        bad = 0xFFFFFFFF
        offs = {}
        for k in range(len(segs)):
            if int(segs["source"][k]) != SRC_STORE:
                continue
            first = int(segs["first"][k])
            e = self.pos.get(ids[first].tobytes())
            if e is None:
                miss += 1
                bad = min(bad, first)
                continue
            lo = self.ends[e - 1] if e else 0
            if self.ends[e] - lo != int(segs["bytes"][k]):
                wrong += 1
                bad = min(bad, first)
            offs[k] = lo
        if not miss and not wrong:
            for k, lo in offs.items():
                segs["src_off"][k] = lo
        return miss, wrong, bad
