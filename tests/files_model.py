"""Python model of the device file layer (include/chunkfs_amd.h, "File layer"),
written for this repository: a dict of span lists over store_model.Model.

It restates the reference's FileLayer (src/system/file_layer.rs) with the one
deviation the layer documents -- a span's offset is its true byte position in
the file -- and keeps the two quirks: the segment take-while that gets stuck on
a span longer than the segment (file_layer.rs:152-175) and the distribution's
dropped last span (file_layer.rs:188-206).
"""
import hashlib

import numpy as np

import store_model as sm

EEXIST, ENOTFOUND, EPERM = -6, -5, -7
SEG_SIZE = 1 << 20


class ModelError(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


class Span:
    __slots__ = ("hash", "offset", "len")

    def __init__(self, h, offset, length):
        self.hash, self.offset, self.len = h, offset, length


class Handle:
    def __init__(self, name, readonly):
        self.name, self.readonly, self.offset = name, readonly, 0


def take_segment(spans, cursor, seg):
    """file_layer.rs:152-175 on a span list: (spans taken, bytes)."""
    taken, total, skipping = [], 0, True
    for sp in spans:
        if skipping and sp.offset < cursor:  # skip_while
            continue
        skipping = False
        total += sp.len  # take_while
        if total > seg:
            total -= sp.len
            break
        taken.append(sp)
    return taken, total


class Files:
    def __init__(self, store=None, seg_size=SEG_SIZE):
        self.store = store if store is not None else sm.Model()
        self.seg = seg_size
        self.files = {}

    # -- name layer -----------------------------------------------------------
    def create(self, name, create_new=True):
        if not create_new and name in self.files:
            raise ModelError(EEXIST)
        self.files[name] = []
        return Handle(name, False)

    def open(self, name, readonly=False):
        if name not in self.files:
            raise ModelError(ENOTFOUND)
        return Handle(name, readonly)

    def exists(self, name):
        return name in self.files

    def list(self):
        return sorted(self.files)

    def clear(self):
        self.files = {}
        self.store = sm.Model()

    def _spans(self, h):
        if h.name not in self.files:
            raise ModelError(ENOTFOUND)
        return self.files[h.name]

    def size(self, h):
        return sum(sp.len for sp in self._spans(h))

    # -- spans ------------------------------------------------------------------
    def append(self, h, data, chunks):
        """Spans of `chunks` ((n, 2) offset/length into `data`), at their true offsets."""
        spans = self._spans(h)
        if h.readonly:
            raise ModelError(EPERM)
        data = np.asarray(data, dtype=np.uint8)
        dig, _ = self.store.put(data, chunks)
        at = sum(sp.len for sp in spans)
        for d, (_, ln) in zip(dig, chunks):
            spans.append(Span(bytes(d), at, int(ln)))
            at += int(ln)
        return len(chunks)

    def append_lengths(self, h, data, lengths):
        """The spans of one write call whose chunks tile `data` with these lengths."""
        lengths = np.asarray(lengths, dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64) if len(lengths) else lengths
        return self.append(h, data, np.stack([offs, lengths], axis=1))

    def _bytes(self, spans):
        return np.frombuffer(b"".join(self.store.db[sp.hash] for sp in spans), dtype=np.uint8)

    def read_complete(self, h):
        return self._bytes(self._spans(h))

    def hashes(self, h):
        return [sp.hash for sp in self._spans(h)]

    def read(self, h):
        taken, total = take_segment(self._spans(h), h.offset, self.seg)
        h.offset += total
        return self._bytes(taken)

    def pread(self, h, offset, length):
        whole = self.read_complete(h)
        return whole[offset:offset + length] if length > 0 else whole[:0]

    def distribution(self, h):
        """digest -> (count, length of the first occurrence) over spans 0 .. n-2,
        keys in order of first occurrence (dicts keep insertion order)."""
        spans = self._spans(h)
        out = {}
        for first, second in zip(spans, spans[1:]):
            if first.hash in out:
                out[first.hash] = (out[first.hash][0] + 1, out[first.hash][1])
            else:
                out[first.hash] = (1, second.offset - first.offset)
        return out


def sha(b):
    return hashlib.sha256(bytes(b)).digest()
