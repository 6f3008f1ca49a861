"""Python model of cdc_file_pack_device and cdc_files_unpack_device
(include/chunkfs_amd.h, "Packs: send and receive"), written for this repository:
the exact byte image and the exact refusal order in plain Python over
files_model.Files / store_model.Model, and the corruptions the CPU and GPU
suites share.

A slot of the device store is a digest here: the model's store is a dict in put
order, one entry per digest, and put order is arena order (gc_model.py).
"""
import hashlib
import struct

import numpy as np

import files_model as fm
import store_model as sm

EINVAL, ENOMEM, ENOTFOUND, EEXIST = -1, -2, -5, -6
MAGIC = b"CDCPACK1"
EXTERNAL = 0xFFFFFFFFFFFFFFFF
HEADER = struct.Struct("<8sIIQQQQQQ")
STATS = ("spans", "chunks", "external_spans", "chunk_bytes", "pack_bytes", "file_size", "chunks_new")

# The checks of an unpack, in the order they run (pack_plan.hpp's PackCheck and pack_check_name).
CHECKS = ("magic", "version", "flags", "section sizes", "total_bytes", "length", "chunk_span order",
          "span_chunk range", "span_chunk of a first occurrence", "span equals its chunk", "chunk_off steps",
          "data_bytes", "file_size", "external_spans")


class PackError(Exception):
    """A refused unpack: the code, and for CDC_EINVAL of a structure check its name and first index."""

    def __init__(self, code, check=None, index=None):
        super().__init__(code, check, index)
        self.code, self.check, self.index = code, check, index


def pad16(n):
    return (int(n) + 15) & ~15


def layout(n_spans, n_chunks, data_bytes):
    """Section offsets {digest, length, span_chunk, chunk_span, chunk_off, data, total}; None past 2^64."""
    names = ("digest", "length", "span_chunk", "chunk_span", "chunk_off", "data")
    if n_spans == 0:  # an empty file is its header
        if n_chunks or data_bytes:
            return None
        return dict({k: 64 for k in names}, total=64)
    sizes = (32 * n_spans, 8 * n_spans, 8 * n_spans, 8 * n_chunks, 8 * (n_chunks + 1), data_bytes)
    out, at = {}, 64
    for name, size in zip(names, sizes):
        out[name] = at
        at += pad16(size)
        if at >= 1 << 64:
            return None
    out["total"] = at
    return out


def carried(files, h, since=None, have=None):
    """(digests of the carried chunks in order of first occurrence, the excluded digests)."""
    spans = files._spans(h)
    excluded = set(sp.hash for sp in files._spans(since)) if since is not None else set()
    if have is not None:
        assert len(have) == len(spans)
        excluded |= {sp.hash for sp, flag in zip(spans, have) if flag}
    order = []
    for sp in spans:
        if sp.hash not in excluded and sp.hash not in order:
            order.append(sp.hash)
    return order, excluded


def pack(files, h, since=None, have=None):
    """The pack of the file behind `h`: (bytes, stats dict)."""
    spans = files._spans(h)
    order, _ = carried(files, h, since, have)
    index = {k: i for i, k in enumerate(order)}
    n, nc = len(spans), len(order)
    first = {}
    for i, sp in enumerate(spans):
        first.setdefault(sp.hash, i)
    chunk_off = [0]
    for k in order:
        chunk_off.append(chunk_off[-1] + pad16(len(files.store.db[k])))
    lay = layout(n, nc, chunk_off[-1])
    span_chunk = [index.get(sp.hash, EXTERNAL) for sp in spans]
    external = sum(1 for c in span_chunk if c == EXTERNAL)
    size = sum(sp.len for sp in spans)
    out = bytearray(lay["total"])
    HEADER.pack_into(out, 0, MAGIC, 1, 0, size, n, nc, external, chunk_off[-1], lay["total"])
    if n:
        for i, sp in enumerate(spans):
            out[lay["digest"] + 32 * i:lay["digest"] + 32 * i + 32] = sp.hash
        struct.pack_into("<%dQ" % n, out, lay["length"], *[sp.len for sp in spans])
        struct.pack_into("<%dQ" % n, out, lay["span_chunk"], *span_chunk)
        struct.pack_into("<%dQ" % nc, out, lay["chunk_span"], *[first[k] for k in order])
        struct.pack_into("<%dQ" % (nc + 1), out, lay["chunk_off"], *chunk_off)
        for k, at in zip(order, chunk_off):
            b = files.store.db[k]
            out[lay["data"] + at:lay["data"] + at + len(b)] = b
    chunk_bytes = sum(len(files.store.db[k]) for k in order)
    return bytes(out), {"spans": n, "chunks": nc, "external_spans": external, "chunk_bytes": chunk_bytes,
                        "pack_bytes": lay["total"], "file_size": size, "chunks_new": 0}


class Parsed:
    """The sections of a pack whose header passed the host's check."""

    def __init__(self, blob, hdr, lay):
        (_, _, _, self.file_size, self.n, self.nc, self.external, self.data_bytes, self.total) = hdr
        self.lay = lay
        n, nc = self.n, self.nc
        self.digest = [bytes(blob[lay["digest"] + 32 * i:lay["digest"] + 32 * i + 32]) for i in range(n)]
        self.length = list(struct.unpack_from("<%dQ" % n, blob, lay["length"])) if n else []
        self.span_chunk = list(struct.unpack_from("<%dQ" % n, blob, lay["span_chunk"])) if n else []
        self.chunk_span = list(struct.unpack_from("<%dQ" % nc, blob, lay["chunk_span"])) if n else []
        self.chunk_off = list(struct.unpack_from("<%dQ" % (nc + 1), blob, lay["chunk_off"])) if n else []
        self.data = blob[lay["data"]:lay["data"] + self.data_bytes]


def check_header(blob, length):
    """The host's part of the structure check: (header tuple, layout) or PackError."""
    hdr = HEADER.unpack_from(blob, 0)
    magic, version, flags, _, n, nc, _, data_bytes, total = hdr
    if magic != MAGIC:
        raise PackError(EINVAL, "magic", 0)
    if version != 1:
        raise PackError(EINVAL, "version", 0)
    if flags != 0:
        raise PackError(EINVAL, "flags", 0)
    lay = layout(n, nc, data_bytes) if nc <= n and data_bytes % 16 == 0 and nc < EXTERNAL else None
    if lay is None or n >= 0xFFFFFFFF:
        raise PackError(EINVAL, "section sizes", 0)
    if lay["total"] != total:
        raise PackError(EINVAL, "total_bytes", 0)
    if total > length:
        raise PackError(EINVAL, "length", 0)
    return hdr, lay


def check_sections(p):
    """The validation kernel: every predicate over every index; the first failing
    check in CHECKS order with its smallest offending index, as the host reports it."""
    n, nc = p.n, p.nc
    bad = {}

    def fail(check, index):
        bad[check] = min(bad.get(check, index), index)

    for k in range(nc):
        i = p.chunk_span[k]
        if not (i < n and (k == 0 or p.chunk_span[k - 1] < i)):
            fail("chunk_span order", k)
        if i < n and p.span_chunk[i] != k:
            fail("span_chunk of a first occurrence", k)
        if k == 0 and p.chunk_off[0] != 0:
            fail("chunk_off steps", k)
        elif i < n:
            a, b = p.chunk_off[k], p.chunk_off[k + 1]
            if p.length[i] > EXTERNAL - 15 or b < a or b - a != pad16(p.length[i]):
                fail("chunk_off steps", k)
    for i in range(n):
        c = p.span_chunk[i]
        if c != EXTERNAL and c >= nc:
            fail("span_chunk range", i)
        if c != EXTERNAL and c < nc and p.chunk_span[c] < n:
            j = p.chunk_span[c]
            if p.length[i] != p.length[j] or p.digest[i] != p.digest[j]:
                fail("span equals its chunk", i)
    if n and not (p.chunk_off[nc] == p.data_bytes and (nc or p.chunk_off[0] == 0)):
        fail("data_bytes", nc)
    if sum(p.length) != p.file_size:
        fail("file_size", n)
    externals = sum(1 for c in p.span_chunk if c == EXTERNAL)
    if externals != p.external:
        fail("external_spans", externals)
    for check in CHECKS:
        if check in bad:
            raise PackError(EINVAL, check, bad[check])


def unpack(files, name, blob, trust=False, length=None, max_chunks=None, arena=None):
    """cdc_files_unpack_device on the model: creates `name` from the first `length`
    bytes of `blob` (default: all) and returns the stats dict, or raises PackError
    by the first check that refuses, in the engine's order.  max_chunks / arena:
    the receiving store's limits (None: large enough)."""
    blob = bytes(blob)
    length = len(blob) if length is None else length
    # 1. arguments
    if length < 64:
        raise PackError(EINVAL, "len < 64")
    if name in files.files:
        raise PackError(EEXIST)
    # 2. structure
    hdr, lay = check_header(blob, length)
    p = Parsed(blob, hdr, lay)
    check_sections(p)
    db = files.store.db
    # 3. externals
    missing = [i for i in range(p.n) if p.span_chunk[i] == EXTERNAL and p.digest[i] not in db]
    if missing:
        raise PackError(ENOTFOUND, "external", missing[0])
    wrong = [i for i in range(p.n) if p.span_chunk[i] == EXTERNAL and len(db[p.digest[i]]) != p.length[i]]
    if wrong:
        raise PackError(EINVAL, "external length", wrong[0])
    # 4. integrity
    chunks = []
    for k in range(p.nc):
        i = p.chunk_span[k]
        chunks.append((p.digest[i], p.data[p.chunk_off[k]:p.chunk_off[k] + p.length[i]]))
    if not trust:
        for k, (dig, b) in enumerate(chunks):
            if hashlib.sha256(b).digest() != dig:
                raise PackError(EINVAL, "hash", k)
    # 5. the put, refused "as if every chunk were new"
    st = files.store.stats()
    if max_chunks is not None and st["unique_chunks"] + p.nc > max_chunks:
        raise PackError(ENOMEM, "max_chunks")
    if arena is not None and st["arena_used"] + sum(pad16(len(b)) for _, b in chunks) > arena:
        raise PackError(ENOMEM, "arena")
    new = 0
    for dig, b in chunks:
        new += dig not in db
        db.setdefault(dig, b)  # first insert wins
    # 6. the table as an append builds it: a span is as long as the chunk stored under its digest
    spans, at = [], 0
    for dig in p.digest:
        spans.append(fm.Span(dig, at, len(db[dig])))
        at += len(db[dig])
    files.files[name] = spans
    files.store.chunks_written += p.n  # every span is an insert, as a write of the content counts them
    files.store.bytes_written += at
    return {"spans": p.n, "chunks": p.nc, "external_spans": p.external, "chunk_bytes": sum(len(b) for _, b in chunks),
            "pack_bytes": p.total, "file_size": at, "chunks_new": new}


# ---- the corruptions both suites share ---------------------------------------------------------
def _set_u64(blob, at, value):
    out = bytearray(blob)
    struct.pack_into("<Q", out, at, value & EXTERNAL)
    return bytes(out)


def _get_u64(blob, at):
    return struct.unpack_from("<Q", blob, at)[0]


def corruptions(good):
    """[(label, bytes, length, trust, code, check)] of a good pack that has at
    least three carried chunks, a span that repeats an earlier one and a unique
    span whose length is no multiple of 16 and not 15 mod 16: one edit each,
    and the check that must refuse it -- no earlier one."""
    hdr, lay = check_header(good, len(good))
    p = Parsed(good, hdr, lay)
    n, nc, total = p.n, p.nc, p.total
    assert nc >= 3 and nc < n
    firsts = set(p.chunk_span)
    dup = next(i for i in range(n) if p.span_chunk[i] != EXTERNAL and i not in firsts)
    other = next(c for c in range(nc) if p.digest[p.chunk_span[c]] != p.digest[dup])
    lone = next(i for i in sorted(firsts) if p.length[i] % 16 not in (0, 15) and p.digest.count(p.digest[i]) == 1)
    flipped = bytearray(good)
    flipped[lay["data"] + p.chunk_off[1]] ^= 0x40  # the first byte of carried chunk 1
    flipped = bytes(flipped)
    swapped = _set_u64(_set_u64(good, lay["chunk_span"], p.chunk_span[1]), lay["chunk_span"] + 8, p.chunk_span[0])
    return [
        ("magic", b"CDCPACK2" + good[8:], total, False, EINVAL, "magic"),
        ("version 2", good[:8] + struct.pack("<I", 2) + good[12:], total, False, EINVAL, "version"),
        ("flags", good[:12] + struct.pack("<I", 1) + good[16:], total, False, EINVAL, "flags"),
        ("total_bytes = len + 1", _set_u64(good, 56, total + 1), total, False, EINVAL, "total_bytes"),
        ("n_spans + 1", _set_u64(good, 24, n + 1), total, False, EINVAL, "total_bytes"),
        ("n_chunks + 1", _set_u64(good, 32, nc + 1), total, False, EINVAL, "total_bytes"),
        ("len 63", good, 63, False, EINVAL, "len < 64"),
        ("len one byte short", good, total - 1, False, EINVAL, "length"),
        ("chunk_span swapped", swapped, total, False, EINVAL, "chunk_span order"),
        ("chunk_span last = n_spans", _set_u64(good, lay["chunk_span"] + 8 * (nc - 1), n), total, False, EINVAL,
         "chunk_span order"),
        ("span_chunk = n_chunks", _set_u64(good, lay["span_chunk"] + 8 * dup, nc), total, False, EINVAL,
         "span_chunk range"),
        ("span_chunk to another digest", _set_u64(good, lay["span_chunk"] + 8 * dup, other), total, False, EINVAL,
         "span equals its chunk"),
        ("chunk_off + 16", _set_u64(good, lay["chunk_off"] + 8, p.chunk_off[1] + 16), total, False, EINVAL,
         "chunk_off steps"),
        ("span_length + 1", _set_u64(good, lay["length"] + 8 * lone, p.length[lone] + 1), total, False, EINVAL,
         "file_size"),
        ("data byte flipped", flipped, total, False, EINVAL, "hash"),
        ("data byte flipped, trusted", flipped, total, True, 0, None),
    ]


# What the corruptions are made from: six hand-made spans, two of them repeats.
CORRUPT_LENGTHS = [100, 32, 100, 17, 32, 1]


def corrupt_source():
    """(data, chunks) of the file whose pack corruptions() edits: spans 2 and 4
    repeat spans 0 and 1."""
    a, b, c, d = (np.random.default_rng(900 + i).integers(0, 256, ln, dtype=np.uint8)
                  for i, ln in enumerate((100, 32, 17, 1)))
    data = np.concatenate([a, b, a, c, b, d])
    lengths = np.asarray(CORRUPT_LENGTHS, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64)
    return data, np.stack([offs, lengths], axis=1)


def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def tiling(lengths):
    lengths = np.asarray(lengths, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64) if len(lengths) else lengths
    return np.stack([offs, lengths], axis=1)


# ---- the shapes both suites use (name -> (data, chunks)); chunks None: the chunker's own -------------
def shapes():
    """Hand-made files: the empty file, one span, span counts around one scan
    block with tiny chunks, every padding length, length-0 spans first, last and
    adjacent, and heavy duplication."""
    out = {"empty": (rand(1, 0), tiling([])), "one span": (rand(2, 777), tiling([777]))}
    for n in (2048, 2049):
        out["%d spans" % n] = (rand(3, 24 * n), tiling([24] * n))
    out["padding lengths"] = (rand(4, 1 + 15 + 16 + 17 + 33), tiling([1, 15, 16, 17, 33]))
    out["length-0 spans"] = (rand(5, 300), np.array([[0, 0], [0, 100], [100, 0], [100, 0], [100, 200], [300, 0]],
                                                     dtype=np.uint64))
    block = rand(6, 8192)
    out["heavy duplication"] = (np.concatenate([block] * 24 + [rand(7, 100)]), tiling([8192] * 24 + [100]))
    return out
