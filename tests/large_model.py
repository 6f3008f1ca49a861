"""Piecewise verification of a chunk list too long to hand to the CPU oracle in
one call (a helper of test_large_model.py and test_gpu_large.py; numpy and
ctypes only, no torch).

Two properties of a chunking rule make a whole list checkable piece by piece
(test_large_model.py asserts both for every rule used this way):

  restart           for any cut c of oracle(d), oracle(d[c:]) is the rest of that
                    list shifted by c;
  prefix stability  the chunks of oracle(d[:m]) that end at or before m - max are
                    chunks of oracle(d).

A list `got` over n bytes is then verified completely by induction: choose
boundaries c_0 = 0 < c_1 < ... among got's own offsets, run the oracle on the
bytes [c_i, min(n, c_{i+1} + 2 max)), and require that its chunks with an
offset below c_{i+1} - c_i equal got's rows between the two boundaries,
shifted, and that c_{i+1} is one of its cuts.  Piece 0 starts at a true cut
(0); each piece proves that the next boundary is a true cut; the last piece
runs to n and is compared whole.  The pieces are independent and the oracle
runs without the GIL, so they go through a thread pool.

Every row of `got` is compared in exactly one piece: the report's `compared`
equals len(got) when the check passes.
"""
import collections
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LINE = 1 << 32
N_BIG = LINE + (16 << 20) + 4099          # ragged: no multiple of 16, of a span or of a segment
EDGE_LENS = (LINE - 1, LINE, LINE + 1)


class Mismatch(AssertionError):
    """A list failed the check: .piece is the piece that found it, .offset the
    absolute offset of the first differing chunk (or of the bad boundary)."""

    def __init__(self, msg, piece, offset):
        super().__init__(msg)
        self.piece, self.offset = piece, offset


Report = collections.namedtuple("Report", "compared pieces bounds")


def pool_size(threads=None):
    return int(threads) if threads else min(16, os.cpu_count() or 1)


def as_rows(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, 2))


def _boundary_rows(got, n, pieces):
    """Row indices k_0 = 0 < k_1 < ...: the first row whose offset is at or
    after each multiple of about n / pieces.  Offsets that run backwards (a
    wrapped list) still give ascending rows: the search is over the running
    maximum."""
    if len(got) == 0:
        return np.zeros(0, dtype=np.int64)
    step = max(1, -(-int(n) // max(1, int(pieces))))
    targets = np.arange(step, int(n), step, dtype=np.uint64)
    k = np.searchsorted(np.maximum.accumulate(got[:, 0]), targets, side="left")
    k = np.unique(k[(k > 0) & (k < len(got))])
    return np.concatenate([[0], k]).astype(np.int64)


def piece_bounds(got, n, pieces):
    """Piece boundaries c_0 = 0 < c_1 < ... taken from got's own offsets."""
    got = as_rows(got)
    return [int(got[k, 0]) for k in _boundary_rows(got, n, pieces)] or [0]


def _first_diff(got, want):
    m = min(len(got), len(want))
    bad = np.flatnonzero((got[:m] != want[:m]).any(axis=1))
    if len(bad):
        return int(bad[0])
    return m if len(got) != len(want) else None


def _row(a, i):
    return [int(x) for x in a[i]] if i < len(a) else None


def _fail(piece, what, i, got, want, base):
    g, w = _row(got, i), _row(want, i)
    at = g[0] if g is not None else w[0] if w is not None else base
    raise Mismatch(f"{what}piece {piece}: first differing chunk at offset {at}: got {g}, oracle {w}", piece, at)


def verify_by_pieces(got, n, fetch, oracle_fn, max_size, pieces=64, threads=None, bounds=None, what=""):
    """Check every row of `got` ((k, 2) offset/length over n bytes) against
    oracle_fn, piece by piece.  fetch(a, b) returns the host bytes [a, b);
    oracle_fn(bytes) the (k, 2) list of one buffer.  `bounds` replaces the
    boundaries piece_bounds would choose; each must be an offset of `got`.
    Raises Mismatch naming the piece, the absolute offset of the first
    differing chunk and both values; returns Report(compared, pieces, bounds)."""
    got, n, max_size = as_rows(got), int(n), int(max_size)
    what = what + ": " if what else ""
    if bounds is None:
        rows = _boundary_rows(got, n, pieces)
    else:
        rows = []
        for i, c in enumerate(bounds):
            k = np.flatnonzero(got[:, 0] == np.uint64(c))
            if not len(k):
                raise Mismatch(f"{what}piece {i}: boundary {int(c)} is not an offset of the list", i, int(c))
            rows.append(int(k[0]))
        rows = np.asarray(rows, dtype=np.int64)
    if len(got) == 0:
        ref = as_rows(oracle_fn(fetch(0, n)))
        if len(ref):
            _fail(0, what, 0, got, ref, 0)
        return Report(0, 1, [0])
    cuts = [int(got[k, 0]) for k in rows]
    if cuts[0] != 0:
        raise Mismatch(f"{what}piece 0: the list starts at offset {cuts[0]}, not 0", 0, cuts[0])
    for i in range(1, len(cuts)):
        if not cuts[i - 1] < cuts[i] < n:
            raise Mismatch(f"{what}piece {i}: boundary {cuts[i]} after {cuts[i - 1]} does not ascend below {n}",
                           i, cuts[i])

    def one(i):
        a, last = cuts[i], i + 1 == len(cuts)
        if last:
            ref = as_rows(oracle_fn(fetch(a, n)))
            mine = got[rows[i]:]
        else:
            span = cuts[i + 1] - a
            ref = as_rows(oracle_fn(fetch(a, min(n, cuts[i + 1] + 2 * max_size))))
            is_cut = bool((ref[:, 0] == np.uint64(span)).any())
            ref = ref[ref[:, 0] < np.uint64(span)]
            mine = got[rows[i]:rows[i + 1]]
        ref = ref + np.array([a, 0], dtype=np.uint64)
        d = _first_diff(mine, ref)
        if d is not None:
            return ("rows", i, d, mine, ref, a)
        if not last and not is_cut:     # equal rows, yet the last of them runs past the boundary
            return ("boundary", i, cuts[i + 1])
        return ("ok", len(mine))

    with ThreadPoolExecutor(max_workers=pool_size(threads)) as pool:
        results = list(pool.map(one, range(len(cuts))))
    compared = 0
    for i, r in enumerate(results):     # in order: the first piece that fails is the one named
        if r[0] == "rows":
            _fail(r[1], what, r[2], r[3], r[4], r[5])
        if r[0] == "boundary":
            raise Mismatch(f"{what}piece {i}: its end, boundary {r[2]}, is not a cut of the oracle's list "
                           f"from {cuts[i]}", i, r[2])
        compared += r[1]
    return Report(compared, len(cuts), cuts)


def verify_window(got, n, fetch, chunks_fn, max_size, at, length, what=""):
    """Check the rows of `got` from its first cut at or after `at` against
    chunks_fn over the `length` bytes from that cut (clipped at n): by the
    restart property chunks_fn sees a true start, by prefix stability its
    chunks that end at or before the window's end - max are chunks of the whole
    list (all of them when the window reaches n).  Returns (the cut, rows
    compared); raises Mismatch (piece = the cut's row)."""
    got, n = as_rows(got), int(n)
    what = what + ": " if what else ""
    k = int(np.searchsorted(np.maximum.accumulate(got[:, 0]), np.uint64(at), side="left")) if len(got) else 0
    if k >= len(got):
        raise Mismatch(f"{what}no cut at or after {at}", k, int(at))
    c = int(got[k, 0])
    b = min(n, c + int(length))
    ref = as_rows(chunks_fn(fetch(c, b)))
    if b < n:
        ref = ref[ref[:, 0] + ref[:, 1] <= np.uint64(max(0, b - c - int(max_size)))]
    ref = ref + np.array([c, 0], dtype=np.uint64)
    mine = got[k:k + len(ref)]
    if b == n:
        mine = got[k:]
    d = _first_diff(mine, ref)
    if d is not None:
        _fail(k, what, d, mine, ref, c)
    return c, len(ref)


def verify_against_longer(got, length, longer, fetch, oracle_fn, max_size, what=""):
    """`got` chunks the first `length` bytes of a stream whose verified list is
    `longer`.  By prefix stability its rows equal `longer`'s up to the last
    chunk that ends at or before length - max; the rest is checked by the
    oracle restarted at that verified cut.  Returns the rows compared."""
    got, longer, length = as_rows(got), as_rows(longer), int(length)
    what = what + ": " if what else ""
    ends = longer[:, 0] + longer[:, 1]
    k = int(np.searchsorted(ends, np.uint64(max(0, length - int(max_size))), side="right"))
    d = _first_diff(got[:k], longer[:k])
    if d is not None:
        _fail(0, what + "shared prefix, ", d, got[:k], longer[:k], 0)
    c = int(ends[k - 1]) if k else 0
    ref = as_rows(oracle_fn(fetch(c, length))) + np.array([c, 0], dtype=np.uint64)
    d = _first_diff(got[k:], ref)
    if d is not None:
        _fail(1, what + "tail, ", d, got[k:], ref, c)
    return k + len(ref)


def sha256_rows(host, rows, threads=None):
    """hashlib SHA-256 of every chunk ((k, 2) offset/length) of the host array
    `host`, as a (k, 32) uint8 array.  hashlib hashes large inputs without the
    GIL, so the rows are shared out over the pool."""
    import hashlib
    rows = as_rows(rows).tolist()
    k, mv = len(rows), memoryview(host)
    out = bytearray(32 * k)

    def work(part):
        for i in range(*part):
            o, ln = rows[i]
            out[32 * i:32 * i + 32] = hashlib.sha256(mv[o:o + ln]).digest()

    t = pool_size(threads)
    step = max(1, -(-k // (4 * t)))
    with ThreadPoolExecutor(max_workers=t) as pool:
        list(pool.map(work, [(a, min(k, a + step)) for a in range(0, k, step)]))
    return np.frombuffer(bytes(out), dtype=np.uint8).reshape(k, 32)


def check_tiling(got, n, min_size, max_size):
    """The size-independent invariants: contiguous from 0, lengths sum to n,
    min <= length <= max for every chunk but the last (<= max)."""
    got = as_rows(got)
    if int(n) == 0:
        assert len(got) == 0
        return
    off, ln = got[:, 0], got[:, 1]
    assert int(off[0]) == 0, f"first offset {int(off[0])}"
    bad = np.flatnonzero(off[1:] != off[:-1] + ln[:-1])
    assert not len(bad), f"row {int(bad[0]) + 1} at {int(off[bad[0] + 1])} does not follow {_row(got, int(bad[0]))}"
    assert int(off[-1]) + int(ln[-1]) == int(n), f"the list ends at {int(off[-1]) + int(ln[-1])}, not {int(n)}"
    assert (ln[:-1] >= np.uint64(min_size)).all() and (ln <= np.uint64(max_size)).all() and int(ln[-1]) > 0
