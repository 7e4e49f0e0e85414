"""A Python model of dsx_read_ranges / dsx_read_plan, written
with bisect: the (range, chunk) pieces of a read, the call's totals, and a
store object that serves IndexPos from host memory."""
import bisect

import numpy as np

BAD_NONE = 0xFFFFFFFF
TOTALS = ("ranges", "bytes", "pieces", "store_bytes", "null_bytes", "missing", "wrong_size", "beyond",
          "first_bad_range", "first_bad_chunk")


def with_dst(ranges):
    """(off, len) packed back to back, or (off, len, dst_off) as given -> triples."""
    out, at = [], 0
    for r in ranges:
        if len(r) == 2:
            out.append((int(r[0]), int(r[1]), at))
            at += int(r[1])
        else:
            out.append(tuple(int(x) for x in r))
    return out


def edge_ranges(ends, start=0):
    """Ranges that begin or end exactly on a chunk end and one byte either side
    of one, one chunk, the whole blob, and the zero-length ranges."""
    ends = [int(e) for e in ends]
    total, n = ends[-1], len(ends)
    out = [(start, total - start), (start, 0), (total, 0)]
    for i in sorted({0, n // 3, n // 2, n - 2, n - 1} & set(range(n))):
        cs, ce = (ends[i - 1] if i else start), ends[i]
        out += [(cs, ce - cs), (ce, 0)]
        for a in (cs - 1, cs, cs + 1):
            for b in (ce - 1, ce, ce + 1):
                if start <= a <= b <= total:
                    out.append((a, b - a))
    return out


def is_beyond(ends, start, off, ln):
    blob_end = int(ends[-1]) if len(ends) else start
    return off < start or off + ln > blob_end


def pieces(ends, ranges, start=0):
    """-> [(range, chunk, chunk_off, dst_off, bytes)] in order; ranges beyond the
    blob and ranges of length 0 give none."""
    ends = [int(e) for e in ends]
    out = []
    for r, (off, ln, dst) in enumerate(with_dst(ranges)):
        if ln == 0 or is_beyond(ends, start, off, ln):
            continue
        first = bisect.bisect_right(ends, off)          # the lowest chunk that ends behind off
        last = bisect.bisect_right(ends, off + ln - 1)  # ... behind the range's last byte
        for i in range(first, last + 1):
            cs = ends[i - 1] if i else start
            lo, hi = max(off, cs), min(off + ln, ends[i])
            if hi > lo:
                out.append((r, i, lo - cs, dst + (lo - off), hi - lo))
    return out


def totals(ends, ids, ranges, stored, start=0, null_id=None, null_size=0):
    """The dsx_read_totals_t of a read.  ids: n 32-byte IDs; stored: {id: size}."""
    ends = [int(e) for e in ends]
    rg = with_dst(ranges)
    t = dict.fromkeys(TOTALS, 0)
    t["ranges"], t["bytes"] = len(rg), sum(ln for _, ln, _ in rg)
    bad_ranges, bad_chunks = [], []
    for r, (off, ln, _) in enumerate(rg):
        if is_beyond(ends, start, off, ln):
            t["beyond"] += 1
            bad_ranges.append(r)
    for r, i, _, _, nbytes in pieces(ends, ranges, start):
        cid = bytes(ids[i])
        size = ends[i] - (ends[i - 1] if i else start)
        t["pieces"] += 1
        if null_id is not None and cid == bytes(null_id):
            bad = size != null_size
            t["wrong_size"] += bad
            t["null_bytes"] += 0 if bad else nbytes
        elif cid not in stored:
            bad = True
            t["missing"] += 1
        else:
            bad = stored[cid] != size
            t["wrong_size"] += bad
            t["store_bytes"] += 0 if bad else nbytes
        if bad:
            bad_ranges.append(r)
            bad_chunks.append(i)
    t["first_bad_range"] = min(bad_ranges, default=BAD_NONE)
    t["first_bad_chunk"] = min(bad_chunks, default=BAD_NONE)
    return t


def expected(blob, ranges, out_len, fill=0xA5):
    """The output of a read that succeeds: blob[off:off+len] at dst_off, `fill` elsewhere."""
    out = np.full(out_len, fill, dtype=np.uint8)
    for off, ln, dst in with_dst(ranges):
        out[dst:dst + ln] = blob[off:off + ln]
    return out


class HostStore:
    """What IndexPos needs of a store, from a dict {id: bytes}: read_ranges with
    readseeker.go's rules (the null chunk from memory, the size check)."""

    def __init__(self, chunks):
        self.chunks = dict(chunks)
        self.calls = 0

    def read_ranges(self, index, ranges, out=None):
        from desync_amd import ChunkMissing, NewNullChunk
        self.calls += 1
        null = NewNullChunk(index.Index.ChunkSizeMax)
        chunks = list(index.Chunks)
        ends = [c.Start + c.Size for c in chunks]
        rg = with_dst(ranges)
        buf = np.zeros(max((d + ln for _, ln, d in rg), default=0), dtype=np.uint8)
        for off, ln, _ in rg:
            if is_beyond(ends, 0, off, ln):
                raise ValueError("a range is beyond the blob")
        for _, i, chunk_off, dst, nbytes in pieces(ends, ranges):
            c = chunks[i]
            if c.ID == null.ID:
                data = null.Data
            elif c.ID not in self.chunks:
                raise ChunkMissing(c.ID)
            else:
                data = self.chunks[c.ID]
            if len(data) != c.Size:
                raise ValueError(f"unexpected size for chunk {c.ID.hex()}")
            buf[dst:dst + nbytes] = np.frombuffer(data, np.uint8)[chunk_off:chunk_off + nbytes]
        return buf, {}
