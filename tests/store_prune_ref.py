"""store_ref's dict-and-bytearray model with dsx_store_prune: which entries
survive, their order, the packed arena, the totals (moved, moved_bytes and
unmatched included) and the ID -> entry map rebuilt."""
import numpy as np

import store_ref


class Store(store_ref.Store):
    def prune(self, ids, remove=False):
        """Keeps the entries whose ID is among ``ids`` (remove: drops them)
        -> dsx_store_prune_totals_t as a dict."""
        ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 32)
        named = {row.tobytes() for row in ids}
        new_ids, new_ends, arena = [], [], bytearray()
        moved = moved_bytes = 0
        for e, cid in enumerate(self.ids):
            if (cid in named) == bool(remove):
                continue
            lo = self.ends[e - 1] if e else 0
            size = self.ends[e] - lo
            if len(arena) != lo:
                moved += 1
                moved_bytes += size
            arena += self.arena[lo:self.ends[e]]
            new_ids.append(cid)
            new_ends.append(len(arena))
        totals = {"entries": len(self.ids), "kept": len(new_ids), "kept_bytes": len(arena),
                  "removed": len(self.ids) - len(new_ids), "removed_bytes": len(self.arena) - len(arena),
                  "moved": moved, "moved_bytes": moved_bytes,
                  "unmatched": sum(1 for cid in named if cid not in self.pos)}
        self.ids, self.ends, self.arena = new_ids, new_ends, arena
        self.pos = {cid: e for e, cid in enumerate(new_ids)}
        return totals
