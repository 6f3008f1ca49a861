"""Oracle and device plumbing shared by the chunk-store tests.

The model of the store is the reference's Database: a dict fed in chunk order
with `setdefault(digest, bytes)` (src/system/database.rs:74-77, the first
insert of a digest wins), with hashlib digests -- the same model
tests/test_gpu_index.py uses for the index's flags.
"""
import hashlib

import numpy as np

GUARD = 64
POISON = 0xA5


def round_up16(n):
    return (int(n) + 15) & ~15


class Model:
    def __init__(self):
        self.db = {}
        self.chunks_written = 0
        self.bytes_written = 0

    def put(self, data, chunks):
        """Insert chunks ((n, 2) offset/length) of `data`; returns ((n, 32) digests, (n,) bool new)."""
        dig = np.empty((len(chunks), 32), dtype=np.uint8)
        new = np.zeros(len(chunks), dtype=bool)
        for i, (o, ln) in enumerate(chunks):
            b = data[int(o):int(o) + int(ln)].tobytes()
            k = hashlib.sha256(b).digest()
            dig[i] = np.frombuffer(k, dtype=np.uint8)
            new[i] = k not in self.db
            self.db.setdefault(k, b)
            self.chunks_written += 1
            self.bytes_written += len(b)
        return dig, new

    def stats(self):
        return {"chunks_written": self.chunks_written, "bytes_written": self.bytes_written,
                "unique_chunks": len(self.db), "unique_bytes": sum(len(b) for b in self.db.values()),
                "arena_used": sum(round_up16(len(b)) for b in self.db.values())}

    def read(self, digests):
        """(concatenated bytes, (n, 2) spans) of the digests in request order."""
        parts = [self.db[bytes(d)] for d in np.asarray(digests, dtype=np.uint8).reshape(-1, 32)]
        lens = np.array([len(p) for p in parts], dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if len(parts) else lens
        return np.frombuffer(b"".join(parts), dtype=np.uint8), np.stack([offs, lens], axis=1)


def assert_stats(store, model):
    st, want = store.stats(), model.stats()
    for k, v in want.items():
        assert st[k] == v, (k, st[k], v)


def dev(arr):
    """A host array on the GPU, complete before any stream reads it."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def dev_chunks(chunks):
    return dev(np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2).view(np.int64))


def put(store, d_data, data_len, chunks, digests):
    """put_device of host chunk / digest lists over a device buffer; returns the new flags."""
    import torch
    n = len(chunks)
    dc, dd = dev_chunks(chunks), dev(digests)
    new = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n_new = store.put_device(d_data.data_ptr(), data_len, dc.data_ptr(), dd.data_ptr(), n, new.data_ptr())
    flags = new[:n].cpu().numpy().astype(bool)
    assert n_new == int(flags.sum())
    return flags


class Guarded:
    """Output buffers for get_device with GUARD poisoned bytes on each side of
    d_out, and a poisoned d_spans."""

    def __init__(self, nbytes, n, shift=0):
        import torch
        self.nbytes, self.n, self.shift = int(nbytes), int(n), int(shift)
        self.buf = torch.full((self.nbytes + 2 * GUARD + shift,), POISON, dtype=torch.uint8, device="cuda")
        self.spans = torch.full((max(n, 1), 2), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    @property
    def out_ptr(self):
        return self.buf.data_ptr() + GUARD + self.shift

    def host(self):
        b = self.buf.cpu().numpy()
        lo, hi = GUARD + self.shift, GUARD + self.shift + self.nbytes
        return b[:lo], b[lo:hi], b[hi:], self.spans[:self.n].cpu().numpy().view(np.uint64)

    def assert_untouched(self):
        a, body, z, sp = self.host()
        assert (a == POISON).all() and (body == POISON).all() and (z == POISON).all()
        assert (sp == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


def get_checked(store, model, digests, shift=0, stream=None):
    """get_device of `digests` into guarded buffers; asserts bytes, spans and guards against the model."""
    want, spans = model.read(digests)
    n = len(digests)
    dd = dev(np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32))
    g = Guarded(want.size, n, shift)
    got = store.get_device(dd.data_ptr(), n, g.out_ptr, want.size, g.spans.data_ptr(), stream)
    assert got == want.size
    a, body, z, sp = g.host()
    assert (a == POISON).all() and (z == POISON).all(), "get_device wrote outside d_out"
    assert (body == want).all()
    assert (sp == spans).all()
    return spans
