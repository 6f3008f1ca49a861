"""Numpy model of the one-launch FastCDC kernel's decomposition
(chunkfs_amd/csrc/small.hip), a helper of test_small_model.py (CPU) and
test_gpu_small_stages.py (GPU).

The kernel splits a stream of at most 4 MiB into 32 KiB blocks.  Every block
writes its records (positions whose windowed hash hits mask_s or mask_l, in
position order) with two precomputed truncated-region results each; the block
that arrives last links the records and walks the chain from offset 0.  The
model restates, from (data, sizes, gear) alone:

  * the records of every block, and the three record budgets (per lane, per
    block, per call) whose overflow makes the kernel fall back;
  * per record, the truncated result of a chunk starting there and of its
    max-cut successor, and WHERE the kernel can know each: in the record's own
    block, in the next block (which holds the region in its LDS), or only in
    the last block (from memory);
  * the chain from offset 0: which starts are records and which are not
    ("heads"), the longest run of record-free max cuts, which starts' regions
    the last block loads from memory, and which of those loads take
    trunc_load's guarded branch for a given number of readable bytes.

The geometry constants are read from small.hpp / small.hip, so the model and
the tests built on it move with the code.
"""
import collections
import os
import re

import numpy as np

import fast_sizes as fs
import oracle
from test_resolve_model import windowed_hash

M64 = (1 << 64) - 1
HIT_S, HIT_L, POS_MASK = 1 << 31, 1 << 30, (1 << 30) - 1
TRUNC_NONE, TRUNC_UNKNOWN = 63, 62


def _const(name, *files):
    for f in files:
        txt = open(os.path.join(oracle.ROOT, "chunkfs_amd", "csrc", f)).read()
        m = re.search(r"constexpr \w+ " + name + r" = ([^;]+);", txt)
        if m:
            expr = re.sub(r"\bk[A-Z]\w*", lambda k: str(_const(k.group(0), *files)), m.group(1))
            return int(eval(re.sub(r"(\d)u\b", r"\1", expr), {"__builtins__": {}}))  # noqa: S307 (digits and operators)
    raise KeyError(name)


BLOCK_BYTES = _const("kBlockBytes", "small.hpp")
MAX_BLOCKS = _const("kMaxBlocks", "small.hpp")
BLOCK_REC_CAP = _const("kBlockRecCap", "small.hpp")
REC_CAP = _const("kRecCap", "small.hpp")
LANE_HITS = _const("kLaneHits", "small.hip", "small.hpp")
ENT_CAP = _const("kEntCap", "small.hip", "small.hpp")
ROUNDS = _const("kRounds", "small.hip", "small.hpp")
PIECE = _const("kPiece", "small.hip", "small.hpp")
LANE_BYTES = 64      # a lane hashes 64 bytes of its wave's piece
WARM = 48            # the stream's first 48 positions have no full window: never records
REGION_SPAN = 52     # a region's <= 47 bytes from its word-aligned first byte: 13 dwords
RUN_LEN = 64         # run_len(): max cuts added per entry and round
GUARD_SPAN = 64      # trunc_load: the aligned bytes its unguarded branch reads

# where a truncated result can be known
UNUSED, NOREGION, OWN, NEXT, LAST = "unused", "noregion", "own", "next", "last"

Regime = collections.namedtuple("Regime", "rem a0 ce re tl")
Trunc = collections.namedtuple("Trunc", "own own_where succ succ_where")
Chain = collections.namedtuple("Chain", "starts is_record heads max_run mem_starts")


def gear_table(gear=None):
    return np.array(oracle._tables()[0] if gear is None else gear, dtype=np.uint64)


class Scan:
    """The windowed-hash hits of one buffer: every stream buf[:n] shares them
    (a position's windowed hash depends on the 48 bytes up to it alone)."""

    def __init__(self, buf, sizes, gear=None):
        self.buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self.sizes = tuple(int(x) for x in sizes)
        self.p = fs.params(*self.sizes)
        self.gear = gear_table(gear)
        self.gear_py = [int(x) for x in self.gear]
        W = windowed_hash(self.buf, self.gear)
        hs = (W & np.uint64(self.p.mask_s)) == 0
        hl = (W & np.uint64(self.p.mask_l)) == 0
        hs[:WARM] = False
        hl[:WARM] = False
        self.pos = np.nonzero(hs | hl)[0]
        self.flags = (hs[self.pos].astype(np.uint32) << np.uint32(31)) | (hl[self.pos].astype(np.uint32) << np.uint32(30))

    def model(self, n=None):
        return Model(self, self.buf.size if n is None else int(n))


class Model:
    """The kernel's stages on the stream scan.buf[:n]."""

    def __init__(self, scan, n):
        assert 0 < n <= scan.buf.size and n <= BLOCK_BYTES * MAX_BLOCKS
        self.s, self.n = scan, n
        self.mn, self.avg, self.mx = scan.sizes
        self.trunc = scan.p.trunc
        k = int(np.searchsorted(scan.pos, n))
        # the flagless record at offset 0 first; nothing at or past n
        self.rpos = np.concatenate([[0], scan.pos[:k]]).astype(np.int64)
        self.rec = np.concatenate([[0], scan.pos[:k].astype(np.uint32) | scan.flags[:k]]).astype(np.uint32)
        self.blocks = (n + BLOCK_BYTES - 1) // BLOCK_BYTES
        self._index = {int(p): i for i, p in enumerate(self.rpos)}
        self._tr = {}

    # -- scan stage --------------------------------------------------------
    def block_records(self, b):
        lo, hi = np.searchsorted(self.rpos, [b * BLOCK_BYTES, (b + 1) * BLOCK_BYTES])
        return self.rec[lo:hi]

    def lane_counts(self):
        """Records per 64-byte lane (index = position // 64)."""
        return np.bincount(self.rpos // LANE_BYTES, minlength=(self.n + LANE_BYTES - 1) // LANE_BYTES)

    def block_counts(self):
        """Per block: its record count as the kernel publishes it
        (BLOCK_REC_CAP + 1 for a block that overflowed a lane or its region)."""
        lanes = self.lane_counts()
        per = BLOCK_BYTES // LANE_BYTES
        out = np.empty(self.blocks, dtype=np.uint32)
        for b in range(self.blocks):
            c = lanes[b * per:(b + 1) * per]
            ovf = c.max(initial=0) > LANE_HITS or c.sum() > BLOCK_REC_CAP
            out[b] = BLOCK_REC_CAP + 1 if ovf else c.sum()
        return out

    def record_fallback(self):
        """The record budget this stream exceeds: "lane", "block", "call" or None."""
        lanes = self.lane_counts()
        per = BLOCK_BYTES // LANE_BYTES
        if lanes.max() > LANE_HITS:
            return "lane"
        if max(int(lanes[b * per:(b + 1) * per].sum()) for b in range(self.blocks)) > BLOCK_REC_CAP:
            return "block"
        return "call" if self.rec.size > REC_CAP else None

    # -- the rule ----------------------------------------------------------
    def regime(self, c):
        rem, center = self.n - c, self.avg
        if rem > self.mx:
            rem = self.mx
        elif rem < center:
            center = rem
        a0, ce, re_ = (self.mn // 2) * 2, (center // 2) * 2, (rem // 2) * 2
        return Regime(rem, a0, ce, re_, min(a0 + self.trunc, re_))

    def live(self, c):
        return self.n - c > self.mn      # else the chunk ends the stream: no result is used

    def trunc_eval(self, c, R=None):
        """First d in [0, tl - a0) whose in-chunk hash (reset at c + a0) hits
        mask_s below the centre / mask_l from it on, else TRUNC_NONE."""
        R = R or self.regime(c)
        g, d8, ms, ml = self.s.gear_py, self.s.buf, self.s.p.mask_s, self.s.p.mask_l
        h = 0
        for d in range(R.tl - R.a0):
            h = ((h << 1) + g[d8[c + R.a0 + d]]) & M64
            if h & (ms if R.a0 + d < R.ce else ml) == 0:
                return d
        return TRUNC_NONE

    def _where(self, a, b):
        """Where the region whose word-aligned first byte is a can be known for
        a record of block b."""
        if a + REGION_SPAN <= (b + 1) * BLOCK_BYTES:
            return OWN
        if b + 1 < self.blocks and a + REGION_SPAN <= (b + 2) * BLOCK_BYTES:
            return NEXT
        return LAST

    def trunc_of(self, c):
        """tneed() and the two evaluation passes for the record at c."""
        if c in self._tr:
            return self._tr[c]
        b = c // BLOCK_BYTES
        if not self.live(c):
            t = Trunc(TRUNC_UNKNOWN, UNUSED, TRUNC_UNKNOWN, UNUSED)
        else:
            R = self.regime(c)
            if R.tl > R.a0:
                own, ow = self.trunc_eval(c, R), self._where((c + R.a0) & ~3, b)
            else:
                own, ow = TRUNC_NONE, NOREGION
            v = c + R.rem
            if R.rem == self.mx and self.n - v > self.mn:   # speculative: the max cut may be the link
                Rv = self.regime(v)
                if Rv.tl > Rv.a0:
                    sv, sw = self.trunc_eval(v, Rv), self._where((v + Rv.a0) & ~3, b)
                else:
                    sv, sw = TRUNC_NONE, NOREGION
            else:
                sv, sw = TRUNC_UNKNOWN, UNUSED
            t = Trunc(own, ow, sv, sw)
        self._tr[c] = t
        return t

    @staticmethod
    def readout_byte(val, where):
        """The byte the scan stage leaves in the record region."""
        return TRUNC_UNKNOWN if where in (UNUSED, LAST) else val

    def block_regions(self, b):
        """The u64 words of block b's record region after the scan stage."""
        out = []
        for r in self.block_records(b):
            t = self.trunc_of(int(r) & POS_MASK)
            lo = self.readout_byte(t.own, t.own_where) | (self.readout_byte(t.succ, t.succ_where) << 8)
            out.append((lo << 32) | int(r))
        return np.array(out, dtype=np.uint64)

    def where_counts(self):
        """How many truncated results (own and successor's) fall in each class."""
        c = collections.Counter()
        for p in self.rpos:
            t = self.trunc_of(int(p))
            c[t.own_where] += 1
            c[t.succ_where] += 1
        return c

    # -- the chain ---------------------------------------------------------
    def step(self, c):
        """(next start, it is the max cut of a record-free window) after a chunk at c."""
        if not self.live(c):
            return self.n, False
        R = self.regime(c)
        t = self.trunc_eval(c, R)
        if t != TRUNC_NONE:
            return c + R.a0 + t, False
        if R.tl < R.re:
            i = int(np.searchsorted(self.rpos, c + R.tl))
            while i < self.rpos.size and self.rpos[i] < c + R.re:
                p = int(self.rpos[i])
                if int(self.rec[i]) & (HIT_S if p - c < R.ce else HIT_L):
                    return p, False
                i += 1
        return c + R.rem, R.rem == self.mx

    def chain(self):
        starts, is_rec, mem = [], [], []
        run = max_run = 0
        c, prev, prev_max = 0, None, False
        while c < self.n:
            rec = c in self._index
            starts.append(c)
            is_rec.append(rec)
            run = run + 1 if (prev_max and not rec) else 0
            max_run = max(max_run, run)
            if self.live(c):
                R = self.regime(c)
                if R.tl > R.a0:
                    if rec:
                        need = self.trunc_of(c).own_where == LAST
                    else:
                        # a head: from memory, unless it is the max-cut successor of a
                        # record whose scan pass already evaluated it
                        known = (prev is not None and prev in self._index and c == prev + self.mx
                                 and self.trunc_of(prev).succ_where in (OWN, NEXT, NOREGION))
                        need = not known
                    if need:
                        mem.append(c)
            prev = c
            c, prev_max = self.step(c)
        heads = [s for s, r in zip(starts, is_rec) if not r]
        return Chain(starts, is_rec, heads, max_run, mem)

    def chunks(self):
        st = self.chain().starts
        off = np.array(st, dtype=np.uint64)
        return np.stack([off, np.diff(np.array(st + [self.n], dtype=np.uint64))], axis=1)

    def guarded(self, c, cap):
        """trunc_load's guarded branch for the region of a chunk starting at c
        with `cap` readable bytes: the aligned 64 bytes around it are not."""
        return (((c + self.regime(c).a0) & ~15) + GUARD_SPAN) > cap

    def guarded_starts(self, cap):
        return [c for c in self.chain().mem_starts if self.guarded(c, cap)]

    # -- the link stage, entry for entry ------------------------------------
    def _link_from(self, c, R, t):
        """(next start, index of the record it is or None): link_from()."""
        if t != TRUNC_NONE:
            return c + R.a0 + t, None       # a truncated hit is never taken for a record
        if R.tl < R.re:
            i = int(np.searchsorted(self.rpos, c + R.tl))
            while i < self.rpos.size and self.rpos[i] < c + R.re:
                p = int(self.rpos[i])
                if int(self.rec[i]) & (HIT_S if p - c < R.ce else HIT_L):
                    return p, i
                i += 1
        return c + R.rem, None

    def _run_len(self, p):
        """run_len(): max cuts from p on while the chunk there has no record
        in its search window, p included, at most RUN_LEN."""
        k, v = 1, p
        while k < RUN_LEN and self.n - v > self.mx:
            R = self.regime(v)
            i = int(np.searchsorted(self.rpos, v + R.tl))
            if i < self.rpos.size and self.rpos[i] < v + R.re:
                break
            v, k = v + self.mx, k + 1
        return k

    def link_stage(self):
        """The last block's link rounds over EVERY record (not the chain's
        alone: a record off the chain whose link is a max cut or a truncated
        hit takes entries too).  Returns (entries used, rounds, failed)."""
        if getattr(self, "_ls", None):
            return self._ls
        n, mn, mx, NONE, END = self.n, self.mn, self.mx, -1, -2
        nrec = int(self.rpos.size)
        tr = [self.trunc_of(int(p)) for p in self.rpos]
        epos = [int(p) for p in self.rpos]
        etr = [self.readout_byte(t.own, t.own_where) for t in tr]
        succ = [self.readout_byte(t.succ, t.succ_where) for t in tr]
        enx, tent = [NONE] * nrec, [0] * nrec
        e0, e1, rnd, fail = 0, nrec, 0, False
        while e0 < e1 and rnd < ROUNDS:
            for e in range(e0, e1):
                if enx[e] != NONE and not tent[e]:
                    continue
                c = epos[e]
                if n - c <= mn:
                    enx[e] = END
                    continue
                R = self.regime(c)
                v = c + R.rem
                spec = R.rem == mx and n - v > mn
                t = etr[e]
                tvk = succ[e] if e < nrec else TRUNC_UNKNOWN
                if t == TRUNC_UNKNOWN:
                    t = self.trunc_eval(c, R)
                if tent[e] and t == TRUNC_NONE:
                    continue
                nx, ri = self._link_from(c, R, t)
                if nx >= n:
                    link = END
                elif ri is not None:
                    link = ri
                else:
                    Rn, tn = self.regime(nx), TRUNC_NONE
                    if n - nx > mn and Rn.tl > Rn.a0:
                        tn = tvk if spec and nx == v and tvk != TRUNC_UNKNOWN else self.trunc_eval(nx, Rn)
                    hl, rk, rp = NONE, 0, 0
                    if n - nx <= mn:
                        hl = END
                    else:
                        nx2, r2 = self._link_from(nx, Rn, tn)
                        if nx2 >= n:
                            hl = END
                        elif r2 is not None:
                            hl = r2
                        else:
                            rp = nx2
                            rk = self._run_len(nx2) if nx2 == nx + Rn.rem and Rn.rem == mx else 1
                    rl, rt = NONE, TRUNC_UNKNOWN
                    if rk == 1:
                        if n - rp <= mn:
                            rl = END
                        else:
                            Rp = self.regime(rp)
                            rt = self.trunc_eval(rp, Rp)
                            nx3, r3 = self._link_from(rp, Rp, rt)
                            rl = END if nx3 >= n else r3 if r3 is not None else NONE
                    b = len(epos)
                    if b + 1 + rk > ENT_CAP:
                        fail, link = True, NONE
                        epos += [0] * (1 + rk)          # (the counter moves all the same)
                        etr += [TRUNC_UNKNOWN] * (1 + rk)
                        enx += [END] * (1 + rk)
                        tent += [0] * (1 + rk)
                    else:
                        epos.append(nx)
                        etr.append(tn)
                        enx.append(hl if hl != NONE else b + 1)
                        tent.append(0)
                        for j in range(rk):
                            epos.append(rp + j * mx)
                            etr.append(rt if rk == 1 and rl != NONE else TRUNC_UNKNOWN)
                            enx.append(b + 2 + j if j + 1 < rk else rl if rk == 1 else NONE)
                            tent.append(1 if j + 1 < rk else 0)
                        link = b
                enx[e], etr[e], tent[e] = link, t, 0
            e0, e1 = e1, min(len(epos), ENT_CAP)
            if fail:
                break
            rnd += 1
        if e0 < e1 or rnd >= ROUNDS:
            fail = True
        self._ls = (len(epos), rnd, fail)
        return self._ls

    def chain_fallback(self):
        """The link stage's budgets: entries (records, heads, runs) within
        ENT_CAP, rounds below ROUNDS."""
        return self.link_stage()[2]

    def fallback(self):
        return self.record_fallback() is not None or self.chain_fallback()


def first_difference(model, counts, regions):
    """Failure report: the first block whose published count or records differ
    from the model, as a string; or that the scan stage was right."""
    want = model.block_counts()
    for b in range(model.blocks):
        if int(counts[b]) != int(want[b]):
            return f"scan stage: block {b} published {int(counts[b])} records, the model has {int(want[b])}"
        if want[b] > BLOCK_REC_CAP:
            continue
        got = regions[b * BLOCK_REC_CAP:b * BLOCK_REC_CAP + int(want[b])]
        exp = model.block_regions(b)
        bad = np.nonzero(got != exp)[0]
        if bad.size:
            i = int(bad[0])
            g, e = int(got[i]), int(exp[i])
            what = "record" if (g ^ e) & 0xFFFFFFFF else "truncated result"
            return (f"scan stage: block {b} record {i}: {what} differs: got {g & POS_MASK} flags {(g >> 30) & 3} "
                    f"t {(g >> 32) & 255}/{(g >> 40) & 255}, model {e & POS_MASK} flags {(e >> 30) & 3} "
                    f"t {(e >> 32) & 255}/{(e >> 40) & 255}")
    return "scan stage right (counts, records and truncated results equal the model): the link stage or the " \
           "chain walk lost the cut"


# ---------------------------------------------------------------------------
# Inputs of tests/test_gpu_small_stages.py, built once and shared (read-only);
# tests/test_small_model.py proves on the CPU that each reaches its path.

KIB, MIB = 1 << 10, 1 << 20
SCAN_SETS = [(4096, 8192, 16384), (1024, 2048, 8192), (1000, 3000, 9000), (32768, 131072, 1048576)]
SCAN_DATA = ["random", "zero_region", "period61"]
SEED = 11
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def set_id(sizes):
    return "-".join(str(x) for x in sizes)


def stream_len(sizes):
    """Ten blocks, the last one partial and the length odd; 3 MiB (96 blocks)
    for the set whose regions lie a whole block after their record."""
    return (3 * MIB if sizes[0] >= BLOCK_BYTES else 320 * KIB) - 37


def scan_input(sizes, name):
    key = ("in", sizes, name)
    if key not in _cache:
        n = stream_len(sizes)
        if name == "period61":
            d = np.resize(oracle.splitmix64_bytes(61, 7), n)
        else:
            d = oracle.splitmix64_bytes(n, SEED + sizes[0])
            if name == "zero_region":     # odd start, one and a half max chunks long
                a = (n // 5) | 1
                d[a:a + sizes[2] + sizes[2] // 2 + 7] = 0
            elif name == "random2":       # other bytes, the same length (ring-slot reuse)
                d = oracle.splitmix64_bytes(n, SEED + sizes[0] + 1)
        _cache[key] = _frozen(np.ascontiguousarray(d))
    return _cache[key]


def ring_slots():
    """HostPath::kRingSlots (host_path.hpp): the pinned slots cdc_chunk_data rotates through."""
    txt = open(os.path.join(oracle.ROOT, "chunkfs_amd", "csrc", "host_path.hpp")).read()
    return int(re.search(r"kRingSlots = (\d+);", txt).group(1))


def scan_of(sizes, name):
    key = ("scan", sizes, name)
    if key not in _cache:
        _cache[key] = Scan(scan_input(sizes, name), sizes)
    return _cache[key]


def ref_of(scan, n, tag):
    """oracle.fastcdc of scan.buf[:n] (tag: the cache name of the scan)."""
    key = ("ref", tag, n)
    if key not in _cache:
        g = None if tag[-1] != "gear0" else scan.gear
        _cache[key] = _frozen(oracle.fastcdc(scan.buf[:n], *scan.sizes, gear=g))
    return _cache[key]


def sweep_start(sizes):
    """The chunk start the stream-end sweep hangs on: the oracle's first one
    past the second block of the random input."""
    scan = scan_of(sizes, "random")
    st = ref_of(scan, scan.buf.size, (sizes, "random"))[:, 0]
    c = int(st[np.searchsorted(st, 2 * BLOCK_BYTES + 1)])
    assert c + sizes[0] + 130 <= scan.buf.size
    return c


def sweep_lengths(sizes):
    """kind -> stream lengths: one byte at a time across the tail-chunk rule
    (n - c = min), a 32 KiB block edge and a 4 KiB piece edge."""
    c, mn = sweep_start(sizes), sizes[0]
    block, piece = 3 * BLOCK_BYTES, 2 * BLOCK_BYTES + 3 * PIECE
    return {"end": list(range(c + mn - 2, c + mn + 131)),
            "block_edge": list(range(block - 70, block + 71)),
            "piece_edge": list(range(piece - 70, piece + 71))}


ALIGN_D = [-2, 0, 1, 2, 17, 47, 48, 63, 64, 130]   # the ten lengths of the alignment test: c + min + d


def align_lengths(sizes):
    c, mn = sweep_start(sizes), sizes[0]
    return [c + mn + d for d in ALIGN_D]


# -- the guarded load ------------------------------------------------------
GUARD_ZERO = [((4096, 8192, 16384), 5), ((1000, 3000, 9000), 9)]   # (sizes, k): k max cuts span three blocks
GUARD_D = list(range(-2, 131))
GUARD_RANDOM_SET, GUARD_RANDOM_SEED = (32768, 131072, 1048576), 218


def zeros_scan(sizes, n):
    key = ("zeros", sizes, n)
    if key not in _cache:
        _cache[key] = Scan(_frozen(np.zeros(n, dtype=np.uint8)), sizes)
    return _cache[key]


def guard_zero_lengths(sizes, k):
    return [k * sizes[2] + sizes[0] + d for d in GUARD_D]


def guard_random():
    """(scan, s, lengths): 1 MiB of random bytes in which the oracle has a
    chunk start s in the last bytes of a block, at least avg after the start
    before it.  s is a record whose region (min = 32 KiB further) ends past
    the next block's bytes: only the last block can evaluate it, from memory;
    the lengths put that region at the stream's end."""
    key = ("guard_random",)
    if key not in _cache:
        sizes = GUARD_RANDOM_SET
        scan = Scan(_frozen(oracle.splitmix64_bytes(MIB, GUARD_RANDOM_SEED)), sizes)
        st = [int(x) for x in ref_of(scan, MIB, (sizes, "guard_random"))[:, 0]]
        s = next(b for a, b in zip(st, st[1:]) if b % BLOCK_BYTES >= BLOCK_BYTES - 44 and b - a >= sizes[1]
                 and b + sizes[0] + 200 <= MIB)
        _cache[key] = (scan, s, [s + sizes[0] + d for d in GUARD_D])
    return _cache[key]


# -- dense records: a GEAR table with entry 0 = 0 ----------------------------
def gear0():
    g = oracle.splitmix64_bytes(256 * 8, 99).view(np.uint64).copy()
    g[0] = 0
    return g


class Dense:
    """Random bytes with zero runs placed so that chosen lanes hold chosen
    numbers of records: with GEAR[0] = 0 the windowed hash is 0, a hit of both
    masks, wherever the last 48 bytes are zero, so a run of 47 + r zero bytes
    ending inside a lane gives that lane r records (checked, and the byte in
    front of the run changed, until the lane holds exactly r and its
    neighbours what they held)."""

    def __init__(self, sizes, n, seed):
        self.sizes, self.gear = sizes, gear0()
        self.p = fs.params(*sizes)
        self.d = oracle.splitmix64_bytes(n, seed)
        self.d[self.d == 0] = 1          # zero bytes only where they are placed

    def _hits(self, lo, hi):
        """Record positions in [lo, hi)."""
        a = max(lo - 47, 0)
        W = windowed_hash(self.d[a:hi], self.gear)[lo - a:]
        hit = ((W & np.uint64(self.p.mask_s)) == 0) | ((W & np.uint64(self.p.mask_l)) == 0)
        return [lo + int(i) for i in np.nonzero(hit)[0] if lo + int(i) >= WARM]

    def lane_count(self, lane):
        return len(self._hits(lane * LANE_BYTES, (lane + 1) * LANE_BYTES))

    def block_count(self, b):
        return len(self._hits(b * BLOCK_BYTES, min((b + 1) * BLOCK_BYTES, self.d.size))) + (1 if b == 0 else 0)

    def put(self, lane, r):
        """r more records in `lane` (which must have room before its byte 8)."""
        lo, hi = (lane - 1) * LANE_BYTES, (lane + 2) * LANE_BYTES
        before = self._hits(lo, hi)
        end = lane * LANE_BYTES + 8 + r      # the run's last byte + 1: records at end - r .. end - 1
        start = end - (47 + r)
        saved = self.d[lo:hi].copy()
        for x in range(1, 256):
            self.d[start:end] = 0
            self.d[start - 1] = x
            after = self._hits(lo, hi)
            new = sorted(set(after) - set(before))
            if len(after) == len(before) + r and new == list(range(end - r, end)):
                return True
            self.d[lo:hi] = saved
        return False

    def fill_block(self, b, target, trunc_hits=False):
        """Runs in every other lane of block b until it holds `target` records.
        Only lanes whose counterpart min bytes on stays free of runs are used:
        a zero byte at c + min would be a truncated hit of the chunk starting
        at the record c, and every such hit takes an entry of the link stage
        (the entry budget is tested on its own)."""
        per = BLOCK_BYTES // LANE_BYTES
        stride = -(-self.sizes[0] // LANE_BYTES)
        lane = b * per + 2
        while True:
            have = self.block_count(b)
            if have >= target:
                assert have == target, (b, have, target)
                return
            if (lane // stride) % 2 and not trunc_hits:
                lane += 2
                continue
            if self.lane_count(lane) == 0 and self.lane_count(lane - 1) == 0:
                self.put(lane, min(LANE_HITS, target - have))     # (False: the next free lane)
            lane += 2
            assert lane < (b + 1) * per - 1, "block full"

    def scan(self):
        return Scan(_frozen(self.d.copy()), self.sizes, self.gear)


def budget_cases():
    """name -> Scan: pairs at the three record budgets (at / one over)."""
    key = ("budget",)
    if key not in _cache:
        sizes, out = (4096, 8192, 16384), {}
        for r in (LANE_HITS, LANE_HITS + 1):
            d = Dense(sizes, 2 * BLOCK_BYTES + 4097, 31)
            lane = next(k for k in range(520, 600) if d.lane_count(k) == 0 and d.lane_count(k - 1) == 0)
            assert d.put(lane, r)
            out[f"lane_{r}"] = d.scan()
        for t in (BLOCK_REC_CAP, BLOCK_REC_CAP + 1):
            d = Dense(sizes, 3 * BLOCK_BYTES + 4097, 32)
            d.fill_block(1, t)
            out[f"block_{t}"] = d.scan()
        for t in (REC_CAP, REC_CAP + 1):
            nb = REC_CAP // (BLOCK_REC_CAP - 40) + 1      # blocks well under their own cap
            d = Dense(sizes, nb * BLOCK_BYTES + 4097, 33)
            left = t - sum(d.block_count(b) for b in range(nb + 1))
            for b in range(nb):
                have = d.block_count(b)
                add = min(left, BLOCK_REC_CAP - 40 - have)
                d.fill_block(b, have + add)
                left -= add
            assert left == 0
            out[f"call_{t}"] = d.scan()
        # the entry budget from the other side: REC_CAP records again, but with
        # zero bytes min after most of them, so that their links are truncated
        # hits and every one of them takes a head entry
        nb = REC_CAP // (BLOCK_REC_CAP - 40) + 1
        d = Dense(sizes, nb * BLOCK_BYTES + 4097, 33)
        for b in range(nb - 1):
            d.fill_block(b, BLOCK_REC_CAP - 40, trunc_hits=True)
        out["entries_over"] = d.scan()
        _cache[key] = out
    return _cache[key]


# -- entry budget and link rounds: zero streams, the default GEAR table ------
HEAD_BUDGET = ENT_CAP - REC_CAP      # entries kept for starts that are not records
ENTRY_CASES = [((4096, 8192, 16384), 100 * 16384 + 5000),     # 100 heads: two rounds
               ((1024, 2048, 8192), 150 * 8192 + 1500),       # 150 heads: three rounds
               ((1024, 2048, 2048), 639 * 2048 + 1500)]       # the most an eligible zero stream reaches


# -- the end regime before a piece that is never loaded ----------------------
def piece_end_cases():
    """[(name, Scan, n)] with GEAR[0] = 0: a record c (a 48-byte zero run ends
    there) whose truncated region c + min .. holds zero bytes -- a hit at its
    first position -- and ends with the stream, 6 bytes on, just below a 4 KiB
    piece edge.  The region's word-aligned 52 bytes reach into the next piece,
    of which the stream has no byte: the block evaluates the region from the
    64 bytes in front of that piece."""
    key = ("piece_end",)
    if key not in _cache:
        sizes, out = (4096, 8192, 16384), []
        for k, j in [(2 * 8 + 3, 1), (2 * 8 + 5, 9), (3 * 8 + 1, 30), (2 * 8 + 7, 40), (2 * 8 + 8, 20)]:
            n = k * PIECE - j
            d = Dense(sizes, n, 40 + k)
            c = n - 6 - sizes[0]
            lane, r = divmod(c, LANE_BYTES)
            d.d[c - 47:c + 1] = 0             # the record at c
            d.d[c + sizes[0]:n] = 0           # its region: zero bytes up to the stream's end
            out.append((f"piece{k}-{j}", d.scan(), n, c))
        _cache[key] = out
    return _cache[key]
