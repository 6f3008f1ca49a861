"""Piecewise verification of a chunk list too long to hand to the CPU oracle in
one call (a helper of test_large_model.py, test_gpu_large.py and
test_gpu_large_later.py; numpy and ctypes only).  At the end: the
expectations of test_gpu_large_later.py -- BLAKE2sp digests of a chunk list,
the index sections of a full pack, the closed forms of the delta cases -- and
the comparison of a pack's data section, the one function here that takes
torch tensors (of any device).

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


# ---- what test_gpu_large_later.py expects ------------------------------------------
# Every function below is checked at small sizes by test_large_model.py against
# the model of its feature (blake2sp_model.oracle, pack_model.pack,
# delta_model.delta); the GPU module evaluates it at N_BIG.

_B2 = dict(digest_size=32, fanout=8, depth=2, leaf_size=0, inner_size=32)


def blake2sp_one(d):
    """BLAKE2sp-256 of one uint8 array.  Leaf g takes the 64-byte blocks 8j + g:
    the chunk's whole 512-byte rows are a (rows, 8, 64) view, and its transpose
    (8, rows, 64), copied once, holds leaf g's share as row g; the ragged last
    row is padded with zeros to one more such row, of which leaf g takes the
    bytes the chunk really holds.  One hashlib call per leaf, each long enough
    to run without the GIL for all but tiny chunks."""
    import hashlib
    d = np.ascontiguousarray(d, dtype=np.uint8).reshape(-1)
    nrow = d.size // 512
    rest = d.size - 512 * nrow
    leaves = np.empty((8, nrow + 1, 64), dtype=np.uint8)
    leaves[:, :nrow] = d[:512 * nrow].reshape(nrow, 8, 64).transpose(1, 0, 2)
    tail = np.zeros(512, dtype=np.uint8)
    tail[:rest] = d[512 * nrow:]
    leaves[:, nrow] = tail.reshape(8, 64)
    flat = leaves.reshape(8, -1)
    mid = [hashlib.blake2s(flat[g, :64 * nrow + min(64, max(0, rest - 64 * g))], node_offset=g, node_depth=0,
                           last_node=(g == 7), **_B2).digest() for g in range(8)]
    return hashlib.blake2s(b"".join(mid), node_offset=0, node_depth=1, last_node=True, **_B2).digest()


def blake2sp_rows(host, rows, threads=None):
    """sha256_rows for BLAKE2sp: the (k, 32) digests of every chunk of `host`."""
    rows = as_rows(rows).tolist()
    k = len(rows)
    out = bytearray(32 * k)

    def work(part):
        for i in range(*part):
            o, ln = rows[i]
            out[32 * i:32 * i + 32] = blake2sp_one(host[o:o + ln])

    t = pool_size(threads)
    step = max(1, -(-k // (4 * t)))
    with ThreadPoolExecutor(max_workers=t) as pool:
        list(pool.map(work, [(a, min(k, a + step)) for a in range(0, k, step)]))
    return np.frombuffer(bytes(out), dtype=np.uint8).reshape(k, 32)


def pad16(x):
    return (np.asarray(x, dtype=np.uint64) + np.uint64(15)) & ~np.uint64(15)


PackIndex = collections.namedtuple("PackIndex", "index layout span_chunk chunk_span chunk_off n_chunks data_bytes "
                                                "chunk_bytes file_size")


def pack_index(rows, digests, flags=0):
    """Everything a full pack (no `since`, no `have`) holds before its data
    section, as a uint8 array: header, digests, span_length, span_chunk,
    chunk_span, chunk_off and the zero padding of each section.  `rows` is the
    file's span list, `digests` its (n, 32) digests; a chunk is carried once, at
    its first span.  .layout holds the section offsets, .chunk_off[k] where
    carried chunk k starts in the data section."""
    import struct
    rows = as_rows(rows)
    n = len(rows)
    dig = np.ascontiguousarray(digests, dtype=np.uint8).reshape(n, 32)
    ln = rows[:, 1]
    size = int(ln.sum())
    if n == 0:
        lay = dict({k: 64 for k in ("digest", "length", "span_chunk", "chunk_span", "chunk_off", "data")}, total=64)
        head = struct.pack("<8sIIQQQQQQ", b"CDCPACK1", 1, flags, 0, 0, 0, 0, 0, 64)
        z = np.zeros(0, dtype=np.uint64)
        return PackIndex(np.frombuffer(head, dtype=np.uint8), lay, z, z, np.zeros(1, dtype=np.uint64), 0, 0, 0, 0)
    _, first, inv = np.unique(dig.view("<u8").reshape(n, 4), axis=0, return_index=True, return_inverse=True)
    chunk_span = np.sort(first).astype(np.uint64)                         # first occurrences, in file order
    span_chunk = np.searchsorted(chunk_span, first[inv.reshape(-1)].astype(np.uint64)).astype(np.uint64)
    nc = len(chunk_span)
    chunk_len = ln[chunk_span.astype(np.int64)]
    chunk_off = np.concatenate([[0], np.cumsum(pad16(chunk_len))]).astype(np.uint64)
    data_bytes = int(chunk_off[-1])
    lay, at = {}, 64
    for name, nbytes in (("digest", 32 * n), ("length", 8 * n), ("span_chunk", 8 * n), ("chunk_span", 8 * nc),
                         ("chunk_off", 8 * (nc + 1)), ("data", data_bytes)):
        lay[name] = at
        at += (nbytes + 15) & ~15
    lay["total"] = at
    out = np.zeros(lay["data"], dtype=np.uint8)
    out[:64] = np.frombuffer(struct.pack("<8sIIQQQQQQ", b"CDCPACK1", 1, flags, size, n, nc, 0, data_bytes, at),
                             dtype=np.uint8)
    out[lay["digest"]:lay["digest"] + 32 * n] = dig.reshape(-1)
    for name, arr in (("length", ln), ("span_chunk", span_chunk), ("chunk_span", chunk_span),
                      ("chunk_off", chunk_off)):
        out[lay[name]:lay[name] + 8 * len(arr)] = np.ascontiguousarray(arr, dtype="<u8").view(np.uint8)
    return PackIndex(out, lay, span_chunk, chunk_span, chunk_off, nc, data_bytes, int(chunk_len.sum()), size)


# The delta cases.  A is a file of `size` bytes; every function returns the ops
# [(b_off, len, a_off)] of cdc_files_delta_device(A, B) (a_off == DELTA_LIT: a
# LITERAL) as the rule of include/chunkfs_amd.h gives them once the table has
# realigned -- which spans the edit re-chunked does not show in the exact answer.
# `e` / `f`: how many bytes the two contents happen to share where a region's
# forward / backward search starts; the caller measures them on the bytes.
DELTA_LIT = (1 << 64) - 1


def common_prefix(a, b):
    """How many leading bytes two arrays share (in blocks: the answer is
    usually a few bytes, the arrays gigabytes)."""
    m, block = min(len(a), len(b)), 1 << 16
    for at in range(0, m, block):
        ne = np.flatnonzero(np.asarray(a[at:min(m, at + block)]) != np.asarray(b[at:min(m, at + block)]))
        if len(ne):
            return at + int(ne[0])
    return m


def common_suffix(a, b):
    """How many trailing bytes two arrays share."""
    m, block = min(len(a), len(b)), 1 << 16
    for at in range(0, m, block):
        k = min(block, m - at)
        x, y = np.asarray(a[len(a) - at - k:len(a) - at]), np.asarray(b[len(b) - at - k:len(b) - at])
        ne = np.flatnonzero(x != y)
        if len(ne):
            return at + k - 1 - int(ne[-1])
    return m


def _ops(*ops):
    return [tuple(int(x) for x in o) for o in ops if o[1]]


def delta_insert(size, p, k):
    """B = A with k bytes inserted at p, the first and the last of which differ
    from A[p] and A[p - 1]."""
    return _ops((0, p, 0), (p, k, DELTA_LIT), (p + k, size - p, p))


def delta_drop_head(size, d, e=0):
    """B = A[d:]; e = common_prefix(A[d:], A): what the region at B's start
    matches under the diagonal 0 before its suffix takes the rest under d."""
    return _ops((0, e, 0), (e, size - d - e, d + e))


def delta_restore_head(size, d, e=0):
    """The reverse: builds A (`size` bytes) out of A[d:]; e as above."""
    return _ops((0, e, 0), (e, d - e, DELTA_LIT), (d, size - d, 0))


def delta_self(size):
    return _ops((0, size, 0))


def delta_truncate(size, t):
    """B = A[:t]."""
    return _ops((0, t, 0))


def delta_extend(size, t, f=0):
    """The reverse: builds A out of A[:t]; f = common_suffix(A, A[:t]): what the
    last bytes match under the closing diagonal t - size."""
    return _ops((0, t, 0), (t, size - t - f, DELTA_LIT), (size - f, f, t - f))


def delta_literal(ops):
    return sum(n for _, n, a in ops if a == DELTA_LIT)


def delta_diagonals(ops):
    """a_off - b_off of every COPY, as Python integers."""
    return [a - b for b, _, a in ops if a != DELTA_LIT]


def masked32(values):
    """What a uint32_t in the place of a uint64_t would have kept."""
    return [int(v) & 0xFFFFFFFF for v in values]


def csrc_const(name, *files):
    """An integer `constexpr` of chunkfs_amd/csrc, read from the source (as
    small_model._const does): digits, shifts and other such constants only."""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chunkfs_amd", "csrc")
    for f in files:
        m = re.search(r"constexpr \w+ " + name + r" = ([^;]+);", open(os.path.join(root, f)).read())
        if m:
            expr = re.sub(r"\bk[A-Z]\w*", lambda k: str(csrc_const(k.group(0), *files)), m.group(1))
            return int(eval(re.sub(r"(\d)u(ll)?\b", r"\1", expr), {"__builtins__": {}}))  # noqa: S307
    raise KeyError(name)


def delta_tiles(nbytes):
    """delta_plan.hpp's delta_tiles: the blocks the edge pass needs for a region."""
    tile = csrc_const("kDeltaTile", "delta_plan.hpp")
    return (int(nbytes) + tile - 1) // tile


def pack_data_mismatch(data, buf, rows, chunk_span, chunk_off, slab=32 << 20):
    """Compares the data section of a full pack (`data`, a torch uint8 tensor)
    with what the index states, on the tensors' own device: carried chunk k is
    the bytes [rows[chunk_span[k]]) of `buf` at chunk_off[k], and every byte
    between its end and chunk_off[k + 1] is zero.  One pass in slabs, every
    byte compared; returns None, or the offset of the first byte that differs."""
    import torch
    dev = data.device
    rows = as_rows(rows)[np.asarray(chunk_span, dtype=np.int64)]
    d_off = torch.from_numpy(np.asarray(chunk_off).astype(np.int64)).to(dev)
    d_src = torch.from_numpy(rows[:, 0].astype(np.int64)).to(dev)
    d_len = torch.from_numpy(rows[:, 1].astype(np.int64)).to(dev)
    nc, total = len(rows), int(data.numel())
    assert total == int(chunk_off[-1]) and len(chunk_off) == nc + 1
    zero = torch.zeros((), dtype=torch.uint8, device=dev)
    for q0 in range(0, total, slab):
        q1 = min(total, q0 + slab)
        q = torch.arange(q0, q1, dtype=torch.int64, device=dev)
        k = (torch.searchsorted(d_off, q, right=True) - 1).clamp_(0, nc - 1)
        r = q - d_off[k]
        inside = r < d_len[k]
        at = (d_src[k] + r).clamp_(0, int(buf.numel()) - 1)      # a pad byte reads some valid byte, unused
        want = torch.where(inside, buf[at], zero)
        bad = want != data[q0:q1]
        if bool(bad.any()):
            return q0 + int(torch.nonzero(bad)[0, 0])
    return None
