"""CPU model of the AE (asymmetric extremum) chunker, written from the rule as
DESIGN.md "AE" and include/chunkfs_amd.h (cdc_create_ae) state it -- not from
the kernels' decomposition into a position bitmap.

  value / cut_ae / chunks(..., fast=False)   the literal byte-serial rule
  chunks(...)                                the same rule with each chunk's scan
                                             done by numpy (running extremum, last
                                             record, first position `window` past
                                             it); tests/test_ae_model.py checks it
                                             against the literal one
  storage_writer                             the reference's StorageWriter loop
                                             (buffer = rest ++
                                             1 MiB segment, chunk_data, the last
                                             chunk carried, flush) over the rule

A buffer is whatever one call is given: bytes at or past its end read as 0.
"""
import numpy as np

MAX, MIN = 0, 1
SEG_SIZE = 1 << 20


def default_window(avg):
    return max(1, int(avg) * 100000 // 171828)


def value(data, i):
    """v(i): the big-endian 32-bit value of the four bytes at i, zeros past the end."""
    n = len(data)
    v = 0
    for j in range(4):
        v = (v << 8) | (int(data[i + j]) if i + j < n else 0)
    return v


def cut_ae(data, s, mn, mx, w, mode):
    """Length of the chunk that starts at s (the literal loop)."""
    n = len(data) - s
    if n <= mn:
        return n
    L = min(n, mx)
    skip = mn - (w + 1) if mn > w + 1 else 0
    m = s + skip
    vm = value(data, m)
    for i in range(m + 1, s + L):
        vi = value(data, i)
        if (vi > vm) if mode == MAX else (vi < vm):
            m, vm = i, vi
        elif i == m + w:
            return i + 1 - s
    return L


def values(data, mode):
    """v(i) of every position as uint32, complemented in Min mode (so that
    "better" is ">" for both modes)."""
    b = np.concatenate([np.asarray(data, dtype=np.uint8), np.zeros(3, dtype=np.uint8)]).astype(np.uint32)
    n = len(b) - 3
    v = (b[0:n] << 24) | (b[1:n + 1] << 16) | (b[2:n + 2] << 8) | b[3:n + 3]
    return ~v if mode == MIN else v


_IDX = np.arange(1 << 16)


def _cut_fast(v, s, mn, mx, w):
    """cut_ae over the prepared values: the scan of one chunk in numpy, over a
    horizon that grows until the cut is inside it."""
    global _IDX
    n = len(v) - s
    if n <= mn:
        return n
    L = min(n, mx)
    skip = mn - (w + 1) if mn > w + 1 else 0
    a, end = s + skip, s + L
    h = min(end, a + 4 * (w + 1))
    while True:
        seg = v[a:h]
        k = len(seg)
        if k > len(_IDX):
            _IDX = np.arange(2 * k)
        idx = _IDX[:k]
        cm = np.maximum.accumulate(seg)
        rec = np.ones(k, dtype=bool)           # position j moves M: strictly better than all before
        rec[1:] = seg[1:] > cm[:-1]
        last = np.maximum.accumulate(np.where(rec, idx, 0))   # M while i = a + j is looked at
        hit = np.flatnonzero(idx - last == w)
        if hit.size:
            return a + int(hit[0]) + 1 - s
        if h == end:
            return L
        h = min(end, a + 4 * (h - a))


def chunks(data, mn, avg, mx, w=None, mode=MAX, fast=True):
    """chunk_data over one buffer: a list of (offset, length) tiling it in order."""
    if w is None:
        w = default_window(avg)
    assert 0 < mn <= avg <= mx and w >= 1 and w + 1 <= mx and mode in (MAX, MIN)
    n = len(data)
    out, s = [], 0
    v = values(data, mode) if fast else None
    while s < n:
        ln = _cut_fast(v, s, mn, mx, w) if fast else cut_ae(data, s, mn, mx, w, mode)
        out.append((s, ln))
        s += ln
    return out


def chunk_array(data, mn, avg, mx, w=None, mode=MAX):
    return np.array(chunks(data, mn, avg, mx, w, mode), dtype=np.uint64).reshape(-1, 2)


def storage_writer(data, mn, avg, mx, w=None, mode=MAX, seg=SEG_SIZE):
    """Span lengths of ChunkStorage::write: StorageWriter::write per `seg` bytes
    (buffer = rest ++ segment; every chunk but the last is a span, the last is
    the new rest), then flush (the rest is the last span)."""
    data = np.asarray(data, dtype=np.uint8)
    spans, rest = [], np.empty(0, dtype=np.uint8)
    for off in range(0, len(data), seg):
        buf = np.concatenate([rest, data[off:off + seg]])
        ch = chunks(buf, mn, avg, mx, w, mode)
        if not ch:
            continue
        spans += [ln for _, ln in ch[:-1]]
        o, ln = ch[-1]
        rest = buf[o:o + ln]
    if len(rest):
        spans.append(len(rest))
    return spans
