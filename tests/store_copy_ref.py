"""The model of dsx_store_copy over two store_ref.Store objects: first
occurrence, dst asked first, and all or nothing for missing IDs and for the
capacity.  The GPU tests compare dst's arena, entries and totals with it byte
for byte."""
import numpy as np

U64_MAX = 0xFFFFFFFFFFFFFFFF
TOTALS = ("total", "copied", "copied_bytes", "present", "repeats", "missing", "first_missing")


def fits(counts, totals):
    """The capacity rule on dst's counts before the call (asked only when nothing is missing)."""
    return (counts["chunks"] + totals["copied"] <= counts["max_chunks"]
            and counts["bytes"] + totals["copied_bytes"] <= counts["arena_bytes"])


def copy(dst, src, ids=None):
    """dsx_store_copy(dst, src, ids); ids None: DSX_COPY_ALL.  -> the totals.
    Raises nothing.  dst changes only if nothing is missing and the copy fits
    (fits() says whether the call returns DSX_E_CAPACITY)."""
    if ids is None:
        ids = list(src.ids)
    else:
        ids = [r.tobytes() for r in np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)]
    seen, new = set(), []
    present = missing = 0
    first_missing = U64_MAX
    for i, cid in enumerate(ids):
        if cid in seen:
            continue
        seen.add(cid)
        if cid in dst.pos:
            present += 1
        elif cid in src.pos:
            new.append(cid)
        else:
            missing += 1
            first_missing = min(first_missing, i)
    copied_bytes = sum(len(src.get(cid)) for cid in new)
    totals = {"total": len(ids), "copied": len(new), "copied_bytes": copied_bytes, "present": present,
              "repeats": len(ids) - len(new) - present - missing, "missing": missing,
              "first_missing": first_missing}
    if missing or not fits(dst.counts(), totals):
        return totals
    for cid in new:
        dst.pos[cid] = len(dst.ids)
        dst.ids.append(cid)
        dst.arena += src.get(cid)
        dst.ends.append(len(dst.arena))
    return totals
