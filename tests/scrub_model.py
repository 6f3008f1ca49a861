"""Python model of the scrub stage (include/chunkfs_amd.h, "Scrub stage"),
written for this repository in the style of store_model.py and files_model.py.

It restates the reference's second stage: the DataContainer that is either a
chunk or a list of target keys (src/system/storage.rs:12-21), the target map,
retrieve through target keys (storage.rs:141-157), CopyScrubber and DumbScrubber
(src/system/scrub.rs:85-129), the storage statistics (storage.rs:193-261) and
the two clears (src/system/mod.rs:271-298).  RechunkScrubber has no counterpart
in the reference: this model is its specification.

The key type is the 32-byte SHA-256 of the value, so the target map is a
Database<Hash, Vec<u8>> -- what a chunk store is.
"""
import hashlib
import math

import numpy as np

import files_model as fm

CHUNK, TARGET = "chunk", "target"


def sha(b):
    return hashlib.sha256(bytes(b)).digest()


def ratio(num, den):
    """num as f64 / den as f64."""
    if den:
        return num / den
    return math.inf if num else math.nan


class Measurements:
    def __init__(self, processed_data=0, data_left=0):
        self.processed_data, self.data_left = processed_data, data_left


class _Retrieved:
    """store.db[digest] for files_model.Files: the bytes a container restores to."""

    def __init__(self, storage):
        self.storage = storage

    def __getitem__(self, digest):
        return self.storage.retrieve([digest])[0]


class Storage:
    """ChunkStorage with a target map: base digest -> (CHUNK, bytes) | (TARGET, [keys])."""

    def __init__(self, target=None):
        self.base = {}
        self.target = {} if target is None else target  # key -> bytes, the first insert wins
        self.size_written = 0
        self.chunks_written = 0
        self.db = _Retrieved(self)

    # -- writes (the same interface as store_model.Model.put) -------------------
    def put(self, data, chunks):
        dig = np.empty((len(chunks), 32), dtype=np.uint8)
        new = np.zeros(len(chunks), dtype=bool)
        for i, (o, ln) in enumerate(chunks):
            b = data[int(o):int(o) + int(ln)].tobytes()
            k = sha(b)
            dig[i] = np.frombuffer(k, dtype=np.uint8)
            new[i] = k not in self.base
            self.base.setdefault(k, (CHUNK, b))  # a digest that exists as a target adds nothing
            self.chunks_written += 1
            self.size_written += len(b)
        return dig, new

    # -- reads -------------------------------------------------------------------
    def retrieve(self, digests):
        out = []
        for d in digests:
            kind, v = self.base[bytes(d)]  # KeyError: NotFound
            out.append(v if kind == CHUNK else b"".join(self.target[k] for k in v))
        return out

    def read(self, digests):
        """(concatenated bytes, (n, 2) spans) of the digests in request order."""
        if not (len(digests) and isinstance(digests[0], bytes)):
            digests = np.asarray(digests, dtype=np.uint8).reshape(-1, 32)
        parts = self.retrieve(digests)
        lens = np.array([len(p) for p in parts], dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if len(parts) else lens
        return np.frombuffer(b"".join(parts), dtype=np.uint8), np.stack([offs, lens], axis=1)

    def iterator(self):
        """digest -> (kind, length the container restores to, [keys])."""
        return {d: (kind, len(self.retrieve([d])[0]), [] if kind == CHUNK else list(v))
                for d, (kind, v) in self.base.items()}

    # -- scrubbers ---------------------------------------------------------------
    def scrub_copy(self):
        m = Measurements()
        for d, (kind, v) in list(self.base.items()):
            if kind == CHUNK:
                self.target.setdefault(d, v)
                m.processed_data += len(v)
            self.base[d] = (TARGET, [d])
        return m

    def scrub_dumb(self):
        return Measurements()

    def scrub_rechunk(self, chunk_data):
        """chunk_data(bytes) -> [(offset, length)] tiling the bytes."""
        m = Measurements()
        for d, (kind, v) in list(self.base.items()):
            if kind != CHUNK:
                continue
            keys = []
            for o, ln in chunk_data(v):
                sub = v[int(o):int(o) + int(ln)]
                keys.append(sha(sub))
                self.target.setdefault(keys[-1], sub)
            self.base[d] = (TARGET, keys)
            m.processed_data += len(v)
        return m

    # -- statistics ----------------------------------------------------------------
    def total_cdc_size(self):
        return sum(len(v) for kind, v in self.base.values() if kind == CHUNK)

    def cdc_dedup_ratio(self):
        return ratio(self.size_written, self.total_cdc_size())

    def average_chunk_size(self):
        return self.total_cdc_size() // len(self.base)

    def full_cdc_dedup_ratio(self):
        return ratio(self.size_written, self.total_cdc_size() + 32 * len(self.base))

    def total_dedup_ratio(self):
        return ratio(self.size_written, self.total_cdc_size() + sum(len(v) for v in self.target.values()))

    def scrub_stats(self):
        targets = [v for kind, v in self.base.values() if kind == TARGET]
        return {"cdc_bytes": self.total_cdc_size(), "chunk_containers": len(self.base) - len(targets),
                "target_containers": len(targets), "keys": sum(len(v) for v in targets),
                "target_bytes": sum(len(v) for v in self.target.values()), "target_values": len(self.target)}

    def stats(self):
        return {"chunks_written": self.chunks_written, "bytes_written": self.size_written,
                "unique_chunks": len(self.base)}

    def clear_database(self):
        self.base.clear()
        self.size_written = self.chunks_written = 0

    def clear_database_full(self):
        self.clear_database()
        self.target.clear()


class FileSystem(fm.Files):
    """files_model.Files over a Storage, with the two clears of mod.rs:271-298."""

    def __init__(self, seg_size=fm.SEG_SIZE, target=None):
        super().__init__(store=Storage(target), seg_size=seg_size)

    def clear(self):  # clear_database: the files and the base; the target map stays
        self.files = {}
        self.store.clear_database()

    def clear_file_system(self):
        self.files = {}
        self.store.clear_database_full()
