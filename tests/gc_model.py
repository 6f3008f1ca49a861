"""Python model of removal and collection (include/chunkfs_amd.h, "Removal and
collection"), written for this repository: store_model.Model and
files_model.Files with remove, collect and retain, and the plain-Python move
planner the engine's group counters are compared with.

The store model is a dict in put order, and put order is arena order: the arena
is the padded containers back to back, a collect keeps that order, and a put
after it appends.  So the model knows every container's arena offset.
"""
import files_model as fm
import store_model as sm

ENOTFOUND = fm.ENOTFOUND
DEFAULT_BOUNCE = 256 << 20


def plan_groups(locs, pads, w_req=DEFAULT_BOUNCE):
    """The move groups of a collect whose survivors, in arena order, lie at
    `locs` with padded lengths `pads`: a list of (a, b, bytes, direct).

    newloc is the exclusive scan of pads and gap[i] = locs[i] - newloc[i] never
    decreases.  The leading run with gap 0 does not move.  From the first moved
    survivor a on: bd is the largest b with bytes(a..b) <= gap[a] (the group may
    be copied arena -> arena: its destination ends at or below its first source),
    bb the largest b with bytes(a..b) <= W.  The direct group is taken when it
    reaches the end or moves at least half of what the bounced one would.
    W = max(longest pad, min(w_req, bytes to move)), rounded up to 16."""
    m = len(locs)
    newloc = [0] * (m + 1)
    for i, p in enumerate(pads):
        newloc[i + 1] = newloc[i] + p
    gaps = [locs[i] - newloc[i] for i in range(m)]
    assert all(g >= 0 for g in gaps) and all(x <= y for x, y in zip(gaps, gaps[1:])), "gaps must not decrease"
    first = next((i for i, g in enumerate(gaps) if g > 0), m)
    moved = newloc[m] - newloc[first]
    W = max(max(pads, default=0), sm.round_up16(min(w_req, moved)))

    def reach(a, limit):
        b = a
        while b < m and newloc[b + 1] - newloc[a] <= limit:
            b += 1
        return b

    groups, a = [], first
    while a < m:
        bd, bb = reach(a, gaps[a]), reach(a, W)
        direct_bytes, bounced_bytes = newloc[bd] - newloc[a], newloc[bb] - newloc[a]
        direct = bd == m or 2 * direct_bytes >= bounced_bytes
        b = bd if direct else bb
        assert b > a
        groups.append((a, b, direct_bytes if direct else bounced_bytes, direct))
        a = b
    return groups


def check_groups_are_safe(locs, pads, groups, w_req=DEFAULT_BOUNCE):
    """The safety argument of DESIGN.md "Removal and collection", executed: runs
    the groups over an arena of container ids and fails if a copy reads a byte
    an earlier copy (or its own launch) has written."""
    m = len(locs)
    newloc = [0]
    for p in pads:
        newloc.append(newloc[-1] + p)
    written_upto = newloc[groups[0][0]] if groups else 0  # everything below is final
    for a, b, nbytes, direct in groups:
        assert nbytes == newloc[b] - newloc[a]
        src_lo = min((locs[i] for i in range(a, b) if pads[i]), default=None)
        if direct:
            # one launch, every piece read and written concurrently: the whole
            # destination range must lie below the whole source range
            assert src_lo is None or newloc[b] <= src_lo, (a, b)
        else:
            assert nbytes <= max(max(pads, default=0), sm.round_up16(w_req))
        # no later survivor's source may be overwritten by this group's write-back
        assert all(newloc[b] <= locs[i] for i in range(b, m) if pads[i]), (a, b)
        assert newloc[a] == written_upto
        written_upto = newloc[b]


class Store(sm.Model):
    """store_model.Model with retain by reference counts."""

    def locs(self):
        """digest -> arena offset: the containers back to back in put order."""
        out, at = {}, 0
        for k, b in self.db.items():
            out[k] = at
            at += sm.round_up16(len(b))
        return out

    def retain_refs(self, refs, w_req=DEFAULT_BOUNCE):
        """Keep the digests with refs[digest] > 0; returns the collect's stats."""
        before, old = self.stats(), self.locs()
        self.db = {k: b for k, b in self.db.items() if refs.get(k, 0) > 0}
        keys = list(self.db)
        pads = [sm.round_up16(len(self.db[k])) for k in keys]
        groups = plan_groups([old[k] for k in keys], pads, w_req)
        self.chunks_written = sum(refs[k] for k in keys)
        self.bytes_written = sum(refs[k] * len(self.db[k]) for k in keys)
        after = self.stats()
        return {"containers_before": before["unique_chunks"], "containers_after": after["unique_chunks"],
                "arena_used_before": before["arena_used"], "arena_used_after": after["arena_used"],
                "bytes_moved": sum(g[2] for g in groups),
                "groups_direct": sum(1 for g in groups if g[3]),
                "groups_bounced": sum(1 for g in groups if not g[3])}

    def retain(self, digests, w_req=DEFAULT_BOUNCE):
        """cdc_store_retain_device: a digest that is not stored refuses the call."""
        refs = {}
        for d in digests:
            k = bytes(d)
            if k not in self.db:
                raise fm.ModelError(ENOTFOUND)
            refs[k] = refs.get(k, 0) + 1
        self.retain_refs(refs, w_req)
        return len(self.db)

    def contains(self, digest):
        return bytes(digest) in self.db


class Files(fm.Files):
    """files_model.Files with remove and collect."""

    def __init__(self, store=None, seg_size=fm.SEG_SIZE):
        super().__init__(store if store is not None else Store(), seg_size)

    def clear(self):
        self.files = {}
        self.store = Store()

    def remove(self, name):
        if name not in self.files:
            raise fm.ModelError(ENOTFOUND)
        del self.files[name]

    def refs(self):
        refs = {}
        for spans in self.files.values():
            for sp in spans:
                refs[sp.hash] = refs.get(sp.hash, 0) + 1
        return refs

    def collect(self, w_req=DEFAULT_BOUNCE):
        return self.store.retain_refs(self.refs(), w_req)
