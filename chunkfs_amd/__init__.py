"""chunkfs_amd -- MI355X-native content-defined chunking behind chunkfs's Chunker API.

Host-side mirror of the reference's chunking surface, over the C ABI in
include/chunkfs_amd.h (libchunkfs_amd.so, hand-written HIP for gfx950):

    reference (Rust)                          here
    Chunk            src/lib.rs:43-66         Chunk
    Chunker trait    src/lib.rs:74-86         Chunker.chunk_data / estimate_chunk_count
    SizeParams       src/chunkers/mod.rs:1    SizeParams
    FastChunker      src/chunkers/fast.rs     FastChunker
    FSChunker        src/chunkers/fixed_size  FSChunker
    Rabin/Ultra/Leap/Seq src/chunkers/*.rs    RabinChunker, UltraChunker, LeapChunker,
                                              SeqChunker (published algorithms; parity
                                              unpinned: cdc-chunkers 0.1.3 absent)
    SuperChunker                              raises NotImplementedError
    (none: this project's own)                AeChunker, AeMode (asymmetric extremum)
    ChunkStorage::write  system/storage.rs    write_spans()
    Database (digest set) system/database.rs  DedupIndex
    Database + retrieve / read_file_complete  ChunkStore
    Scrub, CopyScrubber, DumbScrubber         CopyScrubber, DumbScrubber (system/scrub.rs);
                                              RechunkScrubber is this project's own
    ScrubMeasurements  system/scrub.rs:71-79  ScrubMeasurements
    FileSystem / FileLayer  system/mod.rs,    FileSystem, FileHandle
                            file_layer.rs
    (none: this project's own)                FileSystem.pack / unpack / send / save_file /
                                              load_file, PackStats (packs: send and receive)

Every call runs on the GPU.  There is no CPU fallback: without the built
library or a gfx950 device the constructors raise.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import ALGO, CdcError, cdc_chunk_t, cdc_timing_t, check, lib

KB = 1024
MB = 1024 * KB
GB = 1024 * MB
SEG_SIZE = MB  # src/lib.rs:39

__all__ = [
    "KB", "MB", "GB", "SEG_SIZE", "Chunk", "SizeParams", "Chunker", "FastChunker",
    "FSChunker", "RabinChunker", "SuperChunker", "UltraChunker", "LeapChunker",
    "SeqChunker", "OperationMode", "SeqConfig", "AeChunker", "AeMode", "CdcError", "write_spans", "StreamWriter", "version",
    "DedupIndex", "ChunkStore", "FileSystem", "FileHandle",
    "CopyScrubber", "DumbScrubber", "RechunkScrubber", "ScrubMeasurements", "PackStats",
]


class Chunk:
    """A chunk of processed data: offset and length only (src/lib.rs:41-66)."""

    __slots__ = ("_offset", "_length")

    def __init__(self, offset, length):
        self._offset = int(offset)
        self._length = int(length)

    def offset(self):
        return self._offset

    def length(self):
        return self._length

    def range(self):
        return range(self._offset, self._offset + self._length)

    def __eq__(self, other):
        return isinstance(other, Chunk) and (self._offset, self._length) == (other._offset, other._length)

    def __hash__(self):
        return hash((self._offset, self._length))

    def __repr__(self):
        return f"Chunk {{ offset: {self._offset}, length: {self._length} }}"


class SizeParams:
    """cdc_chunkers::SizeParams {min, avg, max} (re-exported at src/chunkers/mod.rs:1)."""

    __slots__ = ("min", "avg", "max")

    def __init__(self, min, avg, max):  # noqa: A002 -- reference field names
        self.min, self.avg, self.max = int(min), int(avg), int(max)

    def __repr__(self):
        return f"SizeParams {{ min: {self.min}, avg: {self.avg}, max: {self.max} }}"

    def __eq__(self, other):
        return isinstance(other, SizeParams) and (self.min, self.avg, self.max) == (other.min, other.avg, other.max)


def _as_buffer(data):
    """(pointer, length, keepalive) for bytes / bytearray / numpy / memoryview."""
    if isinstance(data, np.ndarray):
        arr = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    else:
        arr = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
    return arr.ctypes.data_as(ctypes.c_void_p), arr.size, arr


def pack_offsets(lengths, align=16):
    """Where buffers of these lengths go in one staging buffer, each at a
    multiple of `align`, in order and without overlap: (offsets, total bytes).
    A buffer of length 0 takes no room."""
    offsets, at = [], 0
    for n in lengths:
        at = -(-at // align) * align
        offsets.append(at)
        at += int(n)
    return offsets, at


class Chunker:
    """The Chunker trait (src/lib.rs:74-86), backed by one GPU handle.

    Not thread-safe, like the reference's Mutex-serialised ChunkerRef.
    """

    _algo = None

    def __init__(self, algo, min, avg, max, device=0):  # noqa: A002
        L = lib()
        h = ctypes.c_void_p()
        rc = L.cdc_create(ALGO[algo], min, avg, max, device, ctypes.byref(h))
        if rc == -4:
            raise NotImplementedError(L.cdc_last_error().decode())
        check(rc)
        self._h = h
        self._pending = []  # first[] arrays of enqueued batches (chunk_batch_device_async)
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().cdc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- trait methods -------------------------------------------------------
    def chunk_array(self, data):
        """chunk_data as an (n, 2) uint64 array of (offset, length)."""
        ptr, n, keep = _as_buffer(data)
        cap = lib().cdc_max_chunk_count(self._h, n)
        out = np.empty((max(cap, 1), 2), dtype=np.uint64)
        cnt = check(lib().cdc_chunk_data(self._h, ptr, n,
                                         out.ctypes.data_as(ctypes.POINTER(cdc_chunk_t)), cap))
        self._drained()
        del keep
        assert cnt <= cap
        return out[:cnt]

    def chunk_and_hash(self, data):
        """chunk_data plus Sha256Hasher::hash (src/hashers.rs:20-36) of every
        chunk, as StorageWriter::write computes them (storage.rs:324-329).
        Returns ((n, 2) uint64 chunks, (n, 32) uint8 SHA-256 digests)."""
        ptr, n, keep = _as_buffer(data)
        cap = lib().cdc_max_chunk_count(self._h, n)
        out = np.empty((max(cap, 1), 2), dtype=np.uint64)
        dig = np.empty((max(cap, 1), 32), dtype=np.uint8)
        cnt = check(lib().cdc_chunk_and_hash(self._h, ptr, n,
                                             out.ctypes.data_as(ctypes.POINTER(cdc_chunk_t)),
                                             dig.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap))
        self._drained()
        del keep
        assert cnt <= cap
        return out[:cnt], dig[:cnt]

    def sha256_chunks_device(self, d_data, d_chunks, n_chunks, d_digests, stream=None):
        """SHA-256 of n_chunks chunks of one device-resident stream (device pointers)."""
        check(lib().cdc_sha256_chunks_device(self._h, ctypes.c_void_p(d_data), ctypes.c_void_p(d_chunks),
                                             n_chunks, ctypes.c_void_p(d_digests),
                                             None if stream is None else ctypes.c_void_p(stream)))

    def sha256_batch_device(self, d_ptrs, first, d_chunks, d_digests, stream=None):
        """SHA-256 of every chunk of a multi-stream batch in one launch
        (cdc_sha256_batch_device): stream i's chunks are d_chunks[first[i] ..
        first[i+1]), offsets relative to d_ptrs[i]."""
        ptrs = np.ascontiguousarray(np.asarray(d_ptrs, dtype=np.uint64))
        fa = np.ascontiguousarray(np.asarray(first, dtype=np.uint64))
        assert fa.size == ptrs.size + 1
        check(lib().cdc_sha256_batch_device(self._h, int(ptrs.size), ctypes.c_void_p(ptrs.ctypes.data),
                                            ctypes.c_void_p(fa.ctypes.data), ctypes.c_void_p(int(d_chunks)),
                                            ctypes.c_void_p(int(d_digests)),
                                            None if stream is None else ctypes.c_void_p(stream)))
        self._drained()

    def hash_batch_device(self, d_ptrs, first, d_chunks, d_digests, hash="sha256", stream=None):  # noqa: A002
        """sha256_batch_device with the hasher named: "sha256" or "blake2sp"
        (cdc_hash_batch_device)."""
        ptrs = np.ascontiguousarray(np.asarray(d_ptrs, dtype=np.uint64))
        fa = np.ascontiguousarray(np.asarray(first, dtype=np.uint64))
        assert fa.size == ptrs.size + 1
        check(lib().cdc_hash_batch_device(self._h, _lib.hash_code(hash), int(ptrs.size),
                                          ctypes.c_void_p(ptrs.ctypes.data), ctypes.c_void_p(fa.ctypes.data),
                                          ctypes.c_void_p(int(d_chunks)), ctypes.c_void_p(int(d_digests)),
                                          None if stream is None else ctypes.c_void_p(stream)))
        self._drained()

    def chunk_data(self, data, empty=None):
        """Chunker::chunk_data (src/lib.rs:80): chunks tiling `data`, appended to `empty`."""
        chunks = [] if empty is None else empty
        chunks.extend(Chunk(int(o), int(l)) for o, l in self.chunk_array(data))
        return chunks

    def estimate_chunk_count(self, data):
        """Chunker::estimate_chunk_count (src/lib.rs:85) -- the reference formula."""
        if isinstance(data, int):
            n = data
        elif isinstance(data, np.ndarray):
            n = data.nbytes
        else:
            n = memoryview(data).nbytes
        return lib().cdc_estimate_chunk_count(self._h, n)

    def max_chunk_count(self, n):
        return lib().cdc_max_chunk_count(self._h, n)

    def __repr__(self):  # impl Debug
        return lib().cdc_describe(self._h).decode()

    # -- device-resident batch (configs 2, 4) --------------------------------
    def chunk_batch_device(self, d_ptrs, lens, d_out_ptr, out_cap, stream=0):
        """Chunk n streams already in HBM.  Returns the host array first[n+1].
        `d_ptrs` / `lens` may be uint64 numpy arrays (no per-call conversion)."""
        ptrs = np.ascontiguousarray(np.asarray(d_ptrs, dtype=np.uint64))
        lens_a = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
        n = int(lens_a.size)
        first = np.empty(n + 1, dtype=np.uint64)
        check(lib().cdc_chunk_batch_device(self._h, n, ctypes.c_void_p(ptrs.ctypes.data),
                                           ctypes.c_void_p(lens_a.ctypes.data), ctypes.c_void_p(int(d_out_ptr)),
                                           out_cap, ctypes.c_void_p(first.ctypes.data),
                                           ctypes.c_void_p(int(stream))))
        self._drained()
        return first

    def chunk_batch_device_async(self, d_ptrs, lens, d_out_ptr, out_cap, stream=0):
        """cdc_chunk_batch_device_async: enqueue the batch (FastCDC batches of
        more than 8 MiB run back to back with no host wait between them).
        Returns its first[n+1] array, filled by batch_sync()."""
        ptrs = np.ascontiguousarray(np.asarray(d_ptrs, dtype=np.uint64))
        lens_a = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
        n = int(lens_a.size)
        first = np.zeros(n + 1, dtype=np.uint64)
        pend = self.__dict__.setdefault("_pending", [])
        pend.append(first)  # the library writes it when the batch is collected
        check(lib().cdc_chunk_batch_device_async(self._h, n, ctypes.c_void_p(ptrs.ctypes.data),
                                                 ctypes.c_void_p(lens_a.ctypes.data),
                                                 ctypes.c_void_p(int(d_out_ptr)), out_cap,
                                                 ctypes.c_void_p(first.ctypes.data), ctypes.c_void_p(int(stream))))
        # At most 3 batches are in flight (a submit collects the batch 3 before
        # it), so older arrays are already written: keep only those 3.
        del pend[:-3]
        return first

    def _drained(self):
        """Every library call but an async submit completes the batches in
        flight first (include/chunkfs_amd.h): their first[] arrays are written."""
        self.__dict__["_pending"] = []

    def batch_sync(self):
        """cdc_batch_sync: complete every enqueued batch; the last one's chunk count."""
        r = check(lib().cdc_batch_sync(self._h))
        self._drained()
        return r

    def batch_max_chunks(self, lens):
        n = len(lens)
        lens_a = (ctypes.c_uint64 * max(n, 1))(*[int(x) for x in lens])
        return lib().cdc_batch_max_chunks(self._h, n, lens_a)

    def last_timing(self):
        t = cdc_timing_t()
        check(lib().cdc_last_timing(self._h, ctypes.byref(t), ctypes.sizeof(t)))
        self._drained()
        return {f: getattr(t, f) for f, _ in cdc_timing_t._fields_}

    def timing_back(self, back):
        """Kernel times of the FastCDC batch `back` calls before the last one
        (0 = last, <= 63; include/chunkfs_amd_debug.h cdc_debug_timing_back)."""
        t = cdc_timing_t()
        check(lib().cdc_debug_timing_back(self._h, back, ctypes.byref(t), ctypes.sizeof(t)))
        return {f: getattr(t, f) for f, _ in cdc_timing_t._fields_}

    def set_gear(self, gear):
        g = np.ascontiguousarray(gear, dtype=np.uint64)
        assert g.shape == (256,)
        check(lib().cdc_set_gear(self._h, g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))


class FastChunker(Chunker):
    """FastCDC 2020 (src/chunkers/fast.rs); default sizes 8/16/64 KiB (fast.rs:17-27)."""

    def __init__(self, sizes=None, device=0):
        sizes = sizes or SizeParams(8 * KB, 16 * KB, 64 * KB)
        self.sizes = sizes
        super().__init__("fast", sizes.min, sizes.avg, sizes.max, device)

    @classmethod
    def default(cls):
        return cls()


class FSChunker(Chunker):
    """Fixed-size chunking (src/chunkers/fixed_size.rs); default 4096 (fixed_size.rs:26-30)."""

    def __init__(self, chunk_size=4096, device=0):
        self.chunk_size = chunk_size
        super().__init__("fixed", chunk_size, 0, 0, device)

    @classmethod
    def default(cls):
        return cls()


class _SizedChunker(Chunker):
    """Common constructor of the chunkers built on the segment-walk engine.

    The reference's Default sizes (SizeParams::{rabin,ultra,leap,seq}_default)
    live in cdc-chunkers 0.1.3, absent offline, so sizes are always explicit.
    Cut rules restate the published algorithms: parity unpinned."""

    _name = None

    def __init__(self, sizes, device=0):
        if sizes is None:
            raise TypeError(f"{self._name}: pass SizeParams explicitly (the crate's defaults are unknown here)")
        self.sizes = sizes
        super().__init__(self._algo, sizes.min, sizes.avg, sizes.max, device)


class RabinChunker(_SizedChunker):
    """Rabin CDC (src/chunkers/rabin.rs:34-56): 48-byte window fingerprint modulo
    a degree-53 polynomial, cut where digest & (2^round(log2 avg) - 1) == 0."""
    _algo, _name = "rabin", "RabinChunker"

    def set_poly(self, poly):
        """Install another polynomial (cdc_set_rabin_poly; degree 9..56): the
        one-call hook for the crate's ChunkerParams once its source exists."""
        check(lib().cdc_set_rabin_poly(self._h, int(poly)))


class UltraChunker(_SizedChunker):
    """UltraCDC (src/chunkers/ultra.rs:30-44): 8-byte Hamming distance to 0xAA..,
    two masks around the normal size, low-entropy (LEST) early cut."""
    _algo, _name = "ultra", "UltraChunker"


class LeapChunker(_SizedChunker):
    """Leap-shaped CDC for LeapChunker (src/chunkers/leap.rs:30-44): 24 eligible
    windows before a cut, leaping past a failing window, as in the Leap-based
    CDC paper.  The window eligibility function is a STAND-IN (a seeded table
    hash against a threshold, include/chunkfs_amd_cdc_params.h), not the
    published one the crate builds from random draws: parity unpinned."""
    _algo, _name = "leap", "LeapChunker"


class OperationMode:
    """seq::OperationMode (re-exported at src/chunkers/seq.rs:3)."""
    Increasing = 0
    Decreasing = 1


class SeqConfig:
    """seq::Config (re-exported at src/chunkers/seq.rs:3); defaults of
    include/chunkfs_amd_cdc_params.h (the crate's field names are unknown)."""

    __slots__ = ("seq_length", "jump_trigger", "jump_size")

    def __init__(self, seq_length=5, jump_trigger=50, jump_size=256):
        self.seq_length, self.jump_trigger, self.jump_size = int(seq_length), int(jump_trigger), int(jump_size)

    def __repr__(self):
        return (f"Config {{ seq_length: {self.seq_length}, jump_trigger: {self.jump_trigger}, "
                f"jump_size: {self.jump_size} }}")


class SeqChunker(Chunker):
    """SeqCDC (src/chunkers/seq.rs:40-55): SeqChunker::new(mode, sizes, config).
    estimate_chunk_count is len / avg (seq.rs:52-54), unlike the others."""

    _algo = "seq"

    def __init__(self, mode=OperationMode.Increasing, sizes=None, config=None, device=0):
        if sizes is None:
            raise TypeError("SeqChunker: pass SizeParams explicitly (the crate's defaults are unknown here)")
        self.mode, self.sizes = int(mode), sizes
        self.config = config or SeqConfig()
        L = lib()
        h = ctypes.c_void_p()
        check(L.cdc_create_seq(self.mode, self.config.seq_length, self.config.jump_trigger,
                               self.config.jump_size, sizes.min, sizes.avg, sizes.max, device, ctypes.byref(h)))
        self._h = h
        self.device = device


class AeMode:
    """Which extremum AE looks for."""
    Max = 0
    Min = 1


def ae_default_window(avg):
    """cdc_ae_default_window (include/chunkfs_amd_cdc_params.h): avg = (e - 1) window."""
    return max(1, int(avg) * 100000 // 171828)


class AeChunker(Chunker):
    """AE, the asymmetric extremum chunker (Zhang et al., INFOCOM 2015; not in
    the reference): a cut `window` positions after the first position whose
    4-byte big-endian value nothing in the window after it beats.  The rule is
    restated in include/chunkfs_amd.h (cdc_create_ae) and DESIGN.md "AE".
    window=None takes the default for sizes.avg."""

    _algo = "ae"

    def __init__(self, sizes=None, window=None, mode=AeMode.Max, device=0):
        if sizes is None:
            raise TypeError("AeChunker: pass SizeParams explicitly")
        self.sizes, self.mode = sizes, int(mode)
        self.window = ae_default_window(sizes.avg) if window is None else int(window)
        if self.window < 1 or self.window >= 1 << 32:  # (0 would ask the C ABI for the default)
            raise CdcError(_lib.CDC_EINVAL, "AeChunker: window must be >= 1")
        L = lib()
        h = ctypes.c_void_p()
        check(L.cdc_create_ae(self.mode, self.window, sizes.min, sizes.avg, sizes.max, device, ctypes.byref(h)))
        self._h = h
        self._pending = []
        self.device = device


class SuperChunker(Chunker):
    """SuperCDC (src/chunkers/supercdc.rs:35-57): NOT implemented.  Its cut rule
    and the cross-call `records` map live in cdc-chunkers 0.1.3, absent offline;
    the constructor raises NotImplementedError (CDC_ENOTSUP)."""

    _algo = "super"

    def __init__(self, sizes=None, device=0):
        s = sizes or SizeParams(2 * KB, 8 * KB, 64 * KB)
        super().__init__("super", s.min, s.avg, s.max, device)


def write_spans(chunker, data, seg_size=SEG_SIZE):
    """ChunkStorage::write (storage.rs:78-103) for one write call (seg_size
    segments through the streaming write path).

    Returns (span lengths in file order, wall seconds of the whole call: host
    copy + H2D + chunking, not the reference's chunk_data-only time).
    """
    ptr, n, keep = _as_buffer(data)
    cap = chunker.max_chunk_count(n) + 1  # spans are chunks: all but the last are >= min
    out = np.empty(max(cap, 1), dtype=np.uint64)
    secs = ctypes.c_double(0.0)
    cnt = check(lib().cdc_fs_write(chunker._h, ptr, n, seg_size,
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), cap,
                                   ctypes.byref(secs)))
    del keep
    assert cnt <= cap
    return out[:cnt], secs.value


class StreamWriter:
    """One file write through the streaming write path (cdc_write_begin /
    cdc_write_segment / cdc_write_finish): ChunkStorage::write_from_stream
    (storage.rs:105-137) with StorageWriter::write per segment and
    StorageWriter::flush at the end (storage.rs:302-383).  Segments are copied
    into a pinned ring and uploaded while the caller continues; drain()
    returns the spans that became final so far (each chunked 256 MiB device
    window), finish() the rest and the wall seconds since begin."""

    def __init__(self, chunker):
        self._ch = chunker
        self._bytes = 0
        check(lib().cdc_write_begin(chunker._h))

    def write(self, segment):
        ptr, n, keep = _as_buffer(segment)
        check(lib().cdc_write_segment(self._ch._h, ptr, n))
        del keep
        self._bytes += n

    def drain(self):
        """Span lengths final since the last drain (cdc_write_drain), file order."""
        cap = self._ch.max_chunk_count(self._bytes) + 1
        out = np.empty(max(cap, 1), dtype=np.uint64)
        cnt = check(lib().cdc_write_drain(self._ch._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), cap))
        return out[:cnt]

    def finish(self):
        cap = self._ch.max_chunk_count(self._bytes) + 1
        out = np.empty(max(cap, 1), dtype=np.uint64)
        secs = ctypes.c_double(0.0)
        cnt = check(lib().cdc_write_finish(self._ch._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), cap,
                                           ctypes.byref(secs)))
        assert cnt <= cap
        return out[:cnt], secs.value


def host_stats(chunker):
    """cdc_debug_host_stats: chunk_data calls, upload s, total s; streaming
    write chunking s and segments; one-launch small-stream calls and how many
    of them fell back to the regular pipeline; chunk lists that failed the
    host guard at first read (guard_trips, expected 0)."""
    v = (ctypes.c_double * 8)()
    check(lib().cdc_debug_host_stats(chunker._h, v, 8))
    return {"calls": int(v[0]), "upload_s": v[1], "total_s": v[2], "write_chunk_s": v[3], "write_segments": int(v[4]),
            "small_calls": int(v[5]), "small_fallbacks": int(v[6]), "guard_trips": int(v[7])}


def host_placement(chunker):
    """cdc_debug_host_placement: the device's PCI address, NUMA node and link;
    the node the pinned ring and chunk list landed on; copy-helper pinning."""
    import json
    buf = ctypes.create_string_buffer(1024)
    n = lib().cdc_debug_host_placement(chunker._h, buf, 1024)
    check(n)
    return json.loads(buf.value.decode())


class DedupIndex:
    """The reference's chunk Database keyed by SHA-256 digest (database.rs:74-87,
    first insert wins) with its storage statistics (storage.rs:193-240), as a
    device hash set on one GPU."""

    def __init__(self, capacity, device=0):
        h = ctypes.c_void_p()
        check(lib().cdc_index_create(device, capacity, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().cdc_index_destroy(h)
            self._h = None

    def insert_device(self, d_digests, d_chunks, n, d_new=None, stream=None):
        """Database::insert of n (digest, chunk) pairs (device pointers), in chunk
        order.  Returns the number of new digests; d_new (optional u8[n]) marks them."""
        return check(lib().cdc_index_insert_device(
            self._h, ctypes.c_void_p(d_digests), ctypes.c_void_p(d_chunks), n,
            None if d_new is None else ctypes.c_void_p(d_new),
            None if stream is None else ctypes.c_void_p(stream)))

    def clear(self):
        check(lib().cdc_index_clear(self._h))

    def stats(self):
        s = _lib.cdc_index_stats_t()
        check(lib().cdc_index_stats(self._h, ctypes.byref(s)))
        d = {f: getattr(s, f) for f, _ in _lib.cdc_index_stats_t._fields_}
        d["cdc_dedup_ratio"] = d["bytes_written"] / d["unique_bytes"] if d["unique_bytes"] else float("nan")
        d["average_chunk_size"] = d["unique_bytes"] // d["unique_chunks"] if d["unique_chunks"] else 0
        return d


def _ptr(p):
    return None if p is None else ctypes.c_void_p(int(p))


def _ratio(num, den):
    """num / den by f64 rules, as the reference's `as f64` divisions: inf when
    only the divisor is 0, nan for 0 / 0."""
    if den:
        return num / den
    return float("inf") if num else float("nan")


class ScrubMeasurements:
    """ScrubMeasurements (scrub.rs:71-79): bytes processed, seconds spent, bytes left untouched."""

    __slots__ = ("processed_data", "running_time", "data_left")

    def __init__(self, processed_data=0, running_time=0.0, data_left=0):
        self.processed_data, self.running_time, self.data_left = int(processed_data), float(running_time), int(data_left)

    def __repr__(self):
        return (f"ScrubMeasurements {{ processed_data: {self.processed_data}, running_time: {self.running_time}s, "
                f"data_left: {self.data_left} }}")


class SpliceStats:
    """cdc_splice_stats_t of one FileSystem.splice: the first span replaced, how
    many spans went and came, where the new cuts met the old ones again (in the
    new file's coordinates), the sizes, the bytes the put stored for first-seen
    chunks, the bytes handed to the chunker and the chunking rounds."""

    FIELDS = ("first_span", "spans_removed", "spans_inserted", "resync_offset", "size_before", "size_after",
              "bytes_new", "window_bytes", "rounds")
    __slots__ = FIELDS

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, int(kw.get(f, 0)))

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self):
        return "SpliceStats { " + ", ".join(f"{f}: {getattr(self, f)}" for f in self.FIELDS) + " }"


class DiffStats:
    """cdc_diff_stats_t of one FileSystem.diff, and the answer itself: .ranges
    is the (n, 2) uint64 array of (offset, length); n_ranges their number;
    bytes_differing the sum of the lengths; bytes_compared the bytes of each
    file whose data was read; bytes_shared the bytes proved equal from the
    tables alone; pieces the intervals the two tables cut [0, common) into."""

    FIELDS = ("n_ranges", "bytes_differing", "bytes_compared", "bytes_shared", "pieces", "size_a", "size_b", "seconds")
    __slots__ = FIELDS + ("ranges",)

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, float(kw.get(f, 0)) if f == "seconds" else int(kw.get(f, 0)))
        self.ranges = np.zeros((0, 2), dtype=np.uint64)

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self):
        return "DiffStats { " + ", ".join(f"{f}: {getattr(self, f)}" for f in self.FIELDS) + " }"


class DeltaStats:
    """cdc_delta_stats_t of one FileSystem.delta, and the script itself: .ops is
    the (n, 3) uint64 array of (b_off, len, a_off) that tiles [0, size_b), a_off
    == DeltaStats.LITERAL for a LITERAL op; n_ops their number; bytes_copy and
    bytes_literal the bytes of either kind; bytes_literal_tables the LITERAL
    bytes before the edges were searched; spans_matched the spans of B whose
    slot A names too; regions the LITERAL regions the tables gave.  .literals
    (literals=True only) is a CUDA uint8 tensor: the LITERAL bytes in op order."""

    LITERAL = _lib.CDC_DELTA_LITERAL
    FIELDS = ("n_ops", "bytes_copy", "bytes_literal", "bytes_literal_tables", "spans_matched", "regions", "size_a",
              "size_b", "seconds")
    __slots__ = FIELDS + ("ops", "literals")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, float(kw.get(f, 0)) if f == "seconds" else int(kw.get(f, 0)))
        self.ops = np.zeros((0, 3), dtype=np.uint64)
        self.literals = None

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self):
        return "DeltaStats { " + ", ".join(f"{f}: {getattr(self, f)}" for f in self.FIELDS) + " }"


class PackStats:
    """cdc_pack_stats_t of one FileSystem.pack / unpack: the file's spans, the
    carried chunks, the spans whose chunk the pack does not carry, the unpadded
    bytes of the carried chunks, the bytes of the whole pack, the file's size,
    and -- unpack only -- the carried chunks the receiver did not hold."""

    FIELDS = ("spans", "chunks", "external_spans", "chunk_bytes", "pack_bytes", "file_size", "chunks_new", "seconds")
    __slots__ = FIELDS

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, float(kw.get(f, 0)) if f == "seconds" else int(kw.get(f, 0)))

    @classmethod
    def _of(cls, s):
        return cls(**{f: getattr(s, f) for f in cls.FIELDS})

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self):
        return "PackStats { " + ", ".join(f"{f}: {getattr(self, f)}" for f in self.FIELDS) + " }"


class CopyScrubber:
    """CopyScrubber (scrub.rs:85-114): every chunk moves to the target map under
    its own hash; the container keeps that one key."""
    _code, chunker = _lib.CDC_SCRUB_COPY, None


class DumbScrubber:
    """DumbScrubber (scrub.rs:116-129): does nothing, all-zero measurements."""
    _code, chunker = _lib.CDC_SCRUB_DUMB, None


class RechunkScrubber:
    """Not in the reference: every stored chunk is chunked again with `chunker`
    (any Chunker of this package, normally a finer one), the sub-chunks are
    deduplicated in the target map under their SHA-256, and the container keeps
    the list of keys."""
    _code = _lib.CDC_SCRUB_RECHUNK

    def __init__(self, chunker):
        self.chunker = chunker


class ChunkStore:
    """The reference's key -> data Database (database.rs:10-36, 74-87, first
    insert wins) with ChunkStorage::retrieve (storage.rs:141-157) and
    FileSystem::read_file_complete (system/mod.rs:149-160) on one GPU: a dedup
    index plus an HBM arena of `arena_bytes` holding each first-seen chunk.
    A refused call (CdcError) changes nothing.  Not thread-safe.

    `hash`: the hasher of the store's digests, "sha256" (the default) or
    "blake2sp" (DESIGN.md "Hashers"); set_hash changes it while the store is
    empty."""

    def __init__(self, max_chunks, arena_bytes, device=0, hash="sha256"):  # noqa: A002
        code = _lib.hash_code(hash)
        h = ctypes.c_void_p()
        check(lib().cdc_store_create(device, max_chunks, arena_bytes, ctypes.byref(h)))
        self._h = h
        self.device = device
        if code != _lib.CDC_HASH_SHA256:
            self.set_hash(code)

    def set_hash(self, hash):  # noqa: A002
        """cdc_store_set_hash: refused (CdcError) unless the store is empty, has
        no target and is no target."""
        check(lib().cdc_store_set_hash(self._h, _lib.hash_code(hash)))

    @property
    def hash(self):
        """The hasher's name: "sha256" or "blake2sp"."""
        code = lib().cdc_store_hash(self._h)
        return next(k for k, v in _lib.HASH.items() if v == code)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().cdc_store_destroy(h)
            self._h = None

    def put_device(self, d_data, data_len, d_chunks, d_digests, n, d_new=None, stream=None):
        """Database::insert of n (digest, chunk of d_data) pairs (device pointers),
        in chunk order.  Returns the number of new digests; d_new (optional
        u8[n]) marks them."""
        return check(lib().cdc_store_put_device(self._h, _ptr(d_data), data_len, _ptr(d_chunks),
                                                _ptr(d_digests), n, _ptr(d_new), _ptr(stream)))

    def put_batch_device(self, d_ptrs, lens, first, d_chunks, d_digests, d_new=None, stream=None):
        """The same for the output of chunk_batch_device + sha256_batch_device:
        stream i's chunks are d_chunks[first[i] .. first[i+1]), offsets relative
        to d_ptrs[i]."""
        ptrs = np.ascontiguousarray(np.asarray(d_ptrs, dtype=np.uint64))
        lens_a = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
        fa = np.ascontiguousarray(np.asarray(first, dtype=np.uint64))
        assert lens_a.size == ptrs.size and fa.size == ptrs.size + 1
        return check(lib().cdc_store_put_batch_device(
            self._h, int(ptrs.size), ctypes.c_void_p(ptrs.ctypes.data), ctypes.c_void_p(lens_a.ctypes.data),
            ctypes.c_void_p(fa.ctypes.data), _ptr(d_chunks), _ptr(d_digests), _ptr(d_new), _ptr(stream)))

    def get_device(self, d_digests, n, d_out, out_cap, d_spans=None, stream=None):
        """ChunkStorage::retrieve(..).concat(): the chunks of n digests, in request
        order, back to back in d_out.  Returns the total byte count; a return >
        out_cap means nothing was written (out_cap = 0 sizes a read).  Raises
        CdcError(CDC_ENOTFOUND) if a digest is absent."""
        return check(lib().cdc_store_get_device(self._h, _ptr(d_digests), n, _ptr(d_out), out_cap,
                                                _ptr(d_spans), _ptr(stream)))

    def contains_device(self, d_digests, n, d_found=None, stream=None):
        """Database::contains for n digests: how many are stored; d_found
        (optional u8[n]) marks them."""
        return check(lib().cdc_store_contains_device(self._h, _ptr(d_digests), n, _ptr(d_found), _ptr(stream)))

    def clear(self):
        check(lib().cdc_store_clear(self._h))

    def retain_device(self, d_digests, n, stream=None):
        """cdc_store_retain_device: keep exactly the containers whose digest is
        among the n given (device pointer, 32 bytes each; duplicates allowed, n =
        0 keeps none), drop the rest and compact the arena in place.  Returns the
        number kept.  CdcError(CDC_ENOTFOUND) for a digest that is not stored,
        CdcError(CDC_ENOTSUP) on a scrubbed store; a refused call changes nothing.
        Every file layer on this store goes stale (include/chunkfs_amd.h,
        "Removal and collection")."""
        return check(lib().cdc_store_retain_device(self._h, _ptr(d_digests), n, _ptr(stream)))

    def retain(self, digests):
        """retain_device for a host array of digests ((n, 32) uint8)."""
        import torch
        dig = np.ascontiguousarray(np.asarray(digests, dtype=np.uint8)).reshape(-1, 32)
        if len(dig) == 0:
            return self.retain_device(None, 0)
        dev = f"cuda:{self.device}"
        d_dig = torch.from_numpy(dig).to(dev)
        torch.cuda.synchronize(dev)
        return self.retain_device(d_dig.data_ptr(), len(dig))

    def stats(self):
        s = _lib.cdc_store_stats_t()
        check(lib().cdc_store_stats(self._h, ctypes.byref(s)))
        d = {f: getattr(s.index, f) for f, _ in _lib.cdc_index_stats_t._fields_}
        d["arena_used"], d["arena_capacity"] = s.arena_used, s.arena_capacity
        if getattr(self, "_target", None) is not None:
            # total_cdc_size counts chunk-kind containers only (storage.rs:193-200)
            cdc = self.scrub_stats()["cdc_bytes"]
            d["cdc_dedup_ratio"] = _ratio(d["bytes_written"], cdc)
            d["average_chunk_size"] = cdc // d["unique_chunks"] if d["unique_chunks"] else 0
            return d
        d["cdc_dedup_ratio"] = d["bytes_written"] / d["unique_bytes"] if d["unique_bytes"] else float("nan")
        d["average_chunk_size"] = d["unique_bytes"] // d["unique_chunks"] if d["unique_chunks"] else 0
        return d

    # -- scrub stage (include/chunkfs_amd.h, "Scrub stage") -----------------------
    def set_target(self, target):
        """ChunkStorage::new_with_scrubber's target_map: `target` (a ChunkStore on
        the same device) becomes this store's target map."""
        check(lib().cdc_store_set_target(self._h, target._h if target is not None else None))
        self._target = target  # kept alive: the library does not own it

    def scrub(self, scrubber, stream=None):
        """ChunkStorage::scrub (storage.rs:180-190) with CopyScrubber(),
        DumbScrubber() or RechunkScrubber(chunker); returns ScrubMeasurements."""
        m = _lib.cdc_scrub_measurements_t()
        ch = scrubber.chunker._h if scrubber.chunker is not None else None
        check(lib().cdc_store_scrub(self._h, scrubber._code, ch, ctypes.byref(m), _ptr(stream)))
        if scrubber.chunker is not None:
            scrubber.chunker._drained()
        return ScrubMeasurements(m.processed_data, m.running_seconds, m.data_left)

    def scrub_stats(self):
        s = _lib.cdc_scrub_stats_t()
        check(lib().cdc_store_scrub_stats(self._h, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in _lib.cdc_scrub_stats_t._fields_}

    def storage_iterator(self):
        """ChunkStorage::iterator (storage.rs:233-235): a list of (digest bytes,
        "chunk" | "target", length the container restores to, [key bytes]), in
        the store's slot order."""
        import torch
        dev = f"cuda:{self.device}"
        n = check(lib().cdc_store_iterate_device(self._h, None, None, None, None, 0, None))
        if n == 0:
            return []
        dig = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        kind = torch.empty(n, dtype=torch.uint8, device=dev)
        ln = torch.empty(n, dtype=torch.int64, device=dev)
        kf = torch.empty(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        assert check(lib().cdc_store_iterate_device(self._h, _ptr(dig.data_ptr()), _ptr(kind.data_ptr()),
                                                    _ptr(ln.data_ptr()), _ptr(kf.data_ptr()), n, None)) == n
        nk = check(lib().cdc_store_keys_device(self._h, None, 0, None))
        keys = torch.empty((max(nk, 1), 32), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        assert check(lib().cdc_store_keys_device(self._h, _ptr(keys.data_ptr()), nk, None)) == nk
        dig, kind, ln, kf, keys = (t.cpu().numpy() for t in (dig, kind, ln, kf, keys))
        assert int(kf[n]) == nk
        return [(dig[i].tobytes(), "target" if kind[i] else "chunk", int(ln[i]),
                 [keys[k].tobytes() for k in range(int(kf[i]), int(kf[i + 1]))]) for i in range(n)]

    def size_distribution(self, adjustment):
        """CDCFixture::size_distribution (bench/mod.rs:218-232): {length //
        adjustment * adjustment: containers}, over every container of the store
        (cdc_store_size_distribution_device).  adjustment == 0 is CDC_EINVAL
        (the reference divides by zero)."""
        import torch
        dev = f"cuda:{self.device}"
        n = check(lib().cdc_store_size_distribution_device(self._h, int(adjustment), None, None, 0, None))
        if n == 0:
            return {}
        sizes = torch.empty(n, dtype=torch.int64, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        assert check(lib().cdc_store_size_distribution_device(self._h, int(adjustment), _ptr(sizes.data_ptr()),
                                                              _ptr(counts.data_ptr()), n, None)) == n
        return dict(zip(sizes.cpu().tolist(), counts.cpu().tolist()))

    # -- host conveniences over the calls above --------------------------------
    def write(self, chunker, data):
        """One file write: chunk and hash `data` (host bytes) with `chunker`, put
        every chunk.  Returns ((n, 2) chunks, (n, 32) digests, (n,) bool new):
        keep the digests, they are the file's spans for read()."""
        import torch
        chunks, dig = chunker.chunk_and_hash(data)
        _, nbytes, arr = _as_buffer(data)
        n = len(chunks)
        if n == 0:
            return chunks, dig, np.zeros(0, dtype=bool)
        dev = f"cuda:{self.device}"
        d_data = torch.from_numpy(arr.copy()).to(dev)
        d_dig = torch.from_numpy(np.ascontiguousarray(dig)).to(dev)
        d_chunks = torch.from_numpy(np.ascontiguousarray(chunks).view(np.int64)).to(dev)
        d_new = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        if self.hash != "sha256":  # (chunk_and_hash is SHA-256 only: hash again with the store's hasher)
            chunker.hash_batch_device([d_data.data_ptr()], [0, n], d_chunks.data_ptr(), d_dig.data_ptr(),
                                      hash=self.hash)
            dig = d_dig.cpu().numpy()
        self.put_device(d_data.data_ptr(), nbytes, d_chunks.data_ptr(), d_dig.data_ptr(), n, d_new.data_ptr())
        return chunks, dig, d_new.cpu().numpy().astype(bool)

    def read(self, digests):
        """FileSystem::read_file_complete: the bytes of the chunks named by
        `digests` ((n, 32) uint8), concatenated, as a host uint8 array."""
        import torch
        dig = np.ascontiguousarray(np.asarray(digests, dtype=np.uint8)).reshape(-1, 32)
        n = len(dig)
        if n == 0:
            return np.zeros(0, dtype=np.uint8)
        dev = f"cuda:{self.device}"
        d_dig = torch.from_numpy(dig).to(dev)
        torch.cuda.synchronize(dev)
        total = self.get_device(d_dig.data_ptr(), n, None, 0)
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        got = self.get_device(d_dig.data_ptr(), n, out.data_ptr(), total)
        assert got == total
        return out[:total].cpu().numpy()


class FileHandle:
    """FileHandle (file_layer.rs:32-41): the file's name, the read cursor, the
    write measurements and -- unless read-only -- the chunker."""

    def __init__(self, fh, name, chunker):
        self._fh, self._name, self.chunker = fh, name, chunker

    def name(self):
        return self._name

    def _close(self):
        if self._fh:
            lib().cdc_file_close(self._fh)
            self._fh = None

    def __del__(self):
        try:
            self._close()
        except Exception:
            pass


class FileSystem:
    """The reference's FileSystem (system/mod.rs) for CDC chunkers, on one GPU:
    named files over a ChunkStore, each file's span table in HBM (the device
    file layer of include/chunkfs_amd.h).  Method names are the reference's.

    One deviation: a span's offset is its true byte position in the file, so
    appending through a re-opened handle works (the reference restarts the
    offsets at the handle's 0, file_layer.rs:136-145).  Two quirks are kept:
    read_from_file returns nothing, cursor stuck, when the span at the cursor is
    longer than the segment; chunk_count_distribution leaves out the last span.
    A refused call (CdcError) changes nothing.  Not thread-safe."""

    def __init__(self, store=None, max_chunks=1 << 16, arena_bytes=256 * MB, seg_size=SEG_SIZE, device=0,
                 hash=None):  # noqa: A002
        """`hash`: the hasher of a store created here ("sha256" when None); with
        `store` given it must be that store's, or None."""
        if store is not None and hash is not None and _lib.hash_code(hash) != _lib.hash_code(store.hash):
            raise ValueError(f"hash={hash!r}, but the store hashes with {store.hash!r}")
        self.store = store if store is not None else ChunkStore(max_chunks, arena_bytes, device,
                                                                hash="sha256" if hash is None else hash)
        self.device = self.store.device
        self.seg_size = int(seg_size)
        h = ctypes.c_void_p()
        check(lib().cdc_files_create(self.store._h, self.seg_size, ctypes.byref(h)))
        self._h = h

    @classmethod
    def new_with_scrubber(cls, scrubber, target=None, max_chunks=1 << 16, arena_bytes=256 * MB,
                          target_max_chunks=1 << 18, target_arena_bytes=256 * MB, seg_size=SEG_SIZE, device=0,
                          hash="sha256"):  # noqa: A002
        """FileSystem::new_with_scrubber (mod.rs:226-239): a file system whose
        store has a target map (`target`, a ChunkStore, created here when None)
        and whose scrub() runs `scrubber`.  `hash`: the hasher of both stores
        (a `target` passed in is set to it, which needs it empty)."""
        store = ChunkStore(max_chunks, arena_bytes, device, hash=hash)
        if target is None:
            target = ChunkStore(target_max_chunks, target_arena_bytes, device, hash=hash)
        elif target.hash != store.hash:
            target.set_hash(hash)
        store.set_target(target)
        fs = cls(store=store, seg_size=seg_size)
        fs.target, fs._scrubber = target, scrubber
        return fs

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().cdc_files_destroy(h)  # before the store it is bound to
            self._h = None

    # -- names and handles -------------------------------------------------------
    def _handle(self, name, chunker, fn, flag):
        fh = ctypes.c_void_p()
        check(fn(self._h, name.encode(), flag, ctypes.byref(fh)))
        return FileHandle(fh, name, chunker)

    def create_file(self, name, chunker, create_new=True):
        """FileSystem::create_file (mod.rs:81-87) passes create_new = true: an
        existing file is replaced by an empty one.  create_new=False is
        FileLayer::create's other branch: CdcError(CDC_EEXIST) if the name exists."""
        return self._handle(name, chunker, lib().cdc_files_create_file, 1 if create_new else 0)

    def open_file(self, name, chunker):
        return self._handle(name, chunker, lib().cdc_files_open, 0)

    def open_file_readonly(self, name):
        return self._handle(name, None, lib().cdc_files_open, 1)

    def file_exists(self, name):
        return bool(check(lib().cdc_files_exists(self._h, name.encode())))

    def list_files(self):
        need = check(lib().cdc_files_list(self._h, None, 0))
        if need == 0:
            return []
        buf = ctypes.create_string_buffer(need)
        assert check(lib().cdc_files_list(self._h, buf, need)) == need
        return [b.decode() for b in buf.raw[:need].split(b"\0")[:-1]]

    def remove_file(self, name):
        """cdc_files_remove: drop the file (host only; collect() reclaims the
        space).  CdcError(CDC_ENOTFOUND) for an unknown name.  Handles to the
        file raise CdcError(CDC_ENOTFOUND) from here on."""
        check(lib().cdc_files_remove(self._h, name.encode()))

    def collect(self, stream=None):
        """cdc_files_collect: keep exactly the containers some file of this
        layer references, compact the arena in place and rewrite every file's
        table.  Returns cdc_collect_stats_t as a dict: containers_before /
        _after, arena_used_before / _after, bytes_moved, groups_direct,
        groups_bounced, seconds."""
        s = _lib.cdc_collect_stats_t()
        check(lib().cdc_files_collect(self._h, ctypes.byref(s), _ptr(stream)))
        return {f: getattr(s, f) for f, _ in _lib.cdc_collect_stats_t._fields_}

    def stat(self, handle):
        s = _lib.cdc_file_stat_t()
        check(lib().cdc_file_stat(handle._fh, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in _lib.cdc_file_stat_t._fields_}

    def close_file(self, handle):
        """WriteMeasurements of the handle's writes: {chunk_time, hash_time} in seconds."""
        st = self.stat(handle)
        handle._close()
        return {"chunk_time": st["chunk_seconds"], "hash_time": st["hash_seconds"]}

    # -- writes ---------------------------------------------------------------------
    def write_to_file(self, handle, data, stream=None):
        """FileSystem::write_to_file (mod.rs:93-110): one chunk_data over the whole
        call, the store's hasher (SHA-256 or BLAKE2sp), put, append -- all on the GPU.  `data` is host bytes
        (uploaded once) or a CUDA uint8 tensor (no host copy).  Returns the
        number of spans appended."""
        import torch
        if handle.chunker is None:  # the library refuses too; this keeps the upload away
            st = self.stat(handle)  # CDC_ENOTFOUND first, as write_to_file checks file_exists first
            del st
            raise CdcError(_lib.CDC_EPERM, "file handle is read-only")
        if isinstance(data, torch.Tensor):
            t = data.contiguous().view(torch.uint8).reshape(-1)
            if not t.is_cuda:
                t = t.to(f"cuda:{self.device}")
        else:
            _, _, arr = _as_buffer(data)
            t = torch.from_numpy(arr.copy()).to(f"cuda:{self.device}")
        if stream is None:
            torch.cuda.synchronize(t.device)  # the call runs on the store's stream, not torch's
        return check(lib().cdc_file_write_device(handle._fh, handle.chunker._h, _ptr(t.data_ptr()), t.numel(),
                                                 _ptr(stream)))

    def write_to_files(self, handles, datas, stream=None):
        """cdc_files_write_batch_device: write_to_file(handles[i], datas[i]) for
        every i, in order, as one call -- one chunk batch, one hash batch, one
        put, one append, and the same files and store as the loop would leave.
        Each of `datas` is host bytes or a CUDA uint8 tensor, mixed freely; the
        host buffers go up in ONE upload, packed at 16-byte-aligned offsets
        (pack_offsets).  All handles write through the chunker of the first.
        Returns the list of span counts.  A refused call (CdcError) changes
        nothing; a read-only handle raises CDC_EPERM before anything is uploaded."""
        import torch
        handles, datas = list(handles), list(datas)
        if len(handles) != len(datas):
            raise ValueError("write_to_files: as many datas as handles")
        for h in handles:
            if h.chunker is None:
                self.stat(h)  # CDC_ENOTFOUND first, as write_to_file
                raise CdcError(_lib.CDC_EPERM, "file handle is read-only")
        if not handles:
            return []
        chunker = handles[0].chunker
        if any(h.chunker is not chunker for h in handles):
            raise ValueError("write_to_files: one chunker per call")
        dev = f"cuda:{self.device}"
        host, tensors = {}, {}
        for i, data in enumerate(datas):
            if isinstance(data, torch.Tensor):
                t = data.contiguous().view(torch.uint8).reshape(-1)
                if t.is_cuda:
                    tensors[i] = t if t.data_ptr() % 16 == 0 or t.numel() == 0 else t.clone()
                else:
                    host[i] = t.numpy()
            else:
                host[i] = _as_buffer(data)[2]
        order = sorted(host)
        offsets, total = pack_offsets([host[i].size for i in order])
        staged = None
        if total:
            staging = np.empty(total, dtype=np.uint8)
            for i, at in zip(order, offsets):
                staging[at:at + host[i].size] = host[i]
            staged = torch.from_numpy(staging).to(dev)
        reqs = (_lib.cdc_fwrite_t * len(handles))()
        for i, h in enumerate(handles):
            reqs[i].fh = h._fh.value
            if i in tensors:
                reqs[i].len = tensors[i].numel()
                reqs[i].d_data = tensors[i].data_ptr() if reqs[i].len else None
        for i, at in zip(order, offsets):
            reqs[i].len = host[i].size
            reqs[i].d_data = staged.data_ptr() + at if reqs[i].len else None
        if stream is None:
            torch.cuda.synchronize(dev)  # the call runs on the store's stream, not torch's
        spans = (ctypes.c_uint64 * len(handles))()
        check(lib().cdc_files_write_batch_device(self._h, chunker._h, len(handles), reqs, spans, _ptr(stream)))
        return [int(x) for x in spans]

    def write_from_stream(self, handle, reader):
        """FileSystem::write_from_stream (mod.rs:116-134): reads `reader` (an
        object with read()) to its end and issues ONE write_to_file.  Chunking
        does not depend on how a write is cut into segments, so
        the spans equal those of the reference's loop over 1 MiB segments.  The
        whole dataset is uploaded at once: it must fit beside the store in HBM."""
        data = reader.read()
        if len(data) == 0:
            return 0
        return self.write_to_file(handle, data)

    def append_device(self, handle, d_data, data_len, d_chunks, d_digests, n, stream=None):
        """cdc_file_append_device: spans chunked and hashed by the caller (device pointers)."""
        return check(lib().cdc_file_append_device(handle._fh, _ptr(d_data), data_len, _ptr(d_chunks),
                                                  _ptr(d_digests), n, _ptr(stream)))

    # -- edits in place ---------------------------------------------------------------
    def splice(self, handle, offset, remove_len, data, stream=None):
        """cdc_file_splice_device: replace the bytes [offset, offset + remove_len)
        of the file with `data` (host bytes, a numpy array or a CUDA uint8
        tensor, as for write_to_file; None or empty inserts nothing), through the
        handle's chunker.  Only the spans from the one that holds offset - 8 to
        the first new cut that falls on an old one are chunked, hashed and stored
        again; the result is span for span the file a single write of the new
        content would have made.  Returns SpliceStats.  A refused call (CdcError)
        changes nothing; the replaced spans' containers stay in the store until
        collect()."""
        import torch
        if handle.chunker is None:  # the library refuses too; this keeps the upload away
            self.stat(handle)  # CDC_ENOTFOUND first, as write_to_file
            raise CdcError(_lib.CDC_EPERM, "file handle is read-only")
        dev = f"cuda:{self.device}"
        if data is None:
            t = torch.empty(0, dtype=torch.uint8, device=dev)
        elif isinstance(data, torch.Tensor):
            t = data.contiguous().view(torch.uint8).reshape(-1)
            if not t.is_cuda:
                t = t.to(dev)
        else:
            t = torch.from_numpy(_as_buffer(data)[2].copy()).to(dev)
        if stream is None:
            torch.cuda.synchronize(dev)  # the call runs on the store's stream, not torch's
        s = _lib.cdc_splice_stats_t()
        got = check(lib().cdc_file_splice_device(handle._fh, handle.chunker._h, int(offset), int(remove_len),
                                                 _ptr(t.data_ptr()) if t.numel() else None, t.numel(),
                                                 ctypes.byref(s), _ptr(stream)))
        if not remove_len and not t.numel():  # nothing to do: the library fills no stats
            size = self.stat(handle)["size"]
            return SpliceStats(size_before=size, size_after=size, resync_offset=int(offset))
        assert got == s.spans_inserted
        return SpliceStats(**{f: getattr(s, f) for f in SpliceStats.FIELDS})

    def pwrite(self, handle, offset, data, stream=None):
        """Overwrite from `offset` on: up to the end of the file in place, the rest
        of `data` extends it (pwrite(2)); offset above the size is refused."""
        size = self.stat(handle)["size"]
        n = data.numel() if hasattr(data, "numel") else _as_buffer(data)[2].size
        return self.splice(handle, offset, max(0, min(int(n), size - int(offset))), data, stream)

    def insert(self, handle, offset, data, stream=None):
        return self.splice(handle, offset, 0, data, stream)

    def delete_range(self, handle, offset, length, stream=None):
        return self.splice(handle, offset, length, None, stream)

    def truncate(self, handle, size, stream=None):
        """Cut the file down to `size` bytes; a size above the file's is refused
        (CDC_EINVAL), as a splice past the end is."""
        have = self.stat(handle)["size"]
        if int(size) > have:
            raise CdcError(_lib.CDC_EINVAL, f"truncate: {size} is above the file's {have} bytes")
        return self.splice(handle, size, have - int(size), None, stream)

    # -- snapshots and diffs ----------------------------------------------------------
    def clone_file(self, src, dst, stream=None):
        """cdc_files_clone: the new file `dst` with a deep copy of `src`'s span
        table -- no put, no arena byte moved, store stats unchanged; an edit of
        either file never shows through the other.  Returns the span count.
        CdcError: CDC_ENOTFOUND for an unknown or stale src, CDC_EEXIST when
        dst exists (dst == src included)."""
        return check(lib().cdc_files_clone(self._h, src.encode(), dst.encode(), _ptr(stream)))

    def diff_device(self, a, b, flags, d_ranges, cap, stats=None, stream=None):
        """cdc_files_diff_device, raw: d_ranges is a device pointer to cap
        cdc_chunk_t, stats a _lib.cdc_diff_stats_t or None.  Returns the number of
        ranges; nothing is written when it exceeds cap."""
        return check(lib().cdc_files_diff_device(a._fh, b._fh, int(flags), _ptr(d_ranges), int(cap),
                                                 ctypes.byref(stats) if stats is not None else None, _ptr(stream)))

    def diff(self, a, b, tables_only=False, stream=None):
        """Where the files behind two handles differ: DiffStats, whose .ranges is
        the (n, 2) uint64 array of maximal runs (offset, length) -- ascending,
        never touching -- over [0, max(size_a, size_b)); bytes past the shorter
        file count as differing.  Pieces whose spans name one store slot at one
        offset are equal by construction and not read.  tables_only: no data is
        read at all and every piece that is not shared counts as differing (a
        superset: the changed-chunks list of a backup)."""
        import torch
        dev = f"cuda:{self.device}"
        flags = _lib.CDC_DIFF_TABLES_ONLY if tables_only else 0
        s = _lib.cdc_diff_stats_t()
        cap = 1024
        while True:
            out = torch.empty((cap, 2), dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            n = self.diff_device(a, b, flags, out.data_ptr(), cap, s, stream)
            if n <= cap:
                break
            cap = n  # the exact count: the files cannot change in between
        r = DiffStats(n_ranges=s.ranges, **{f: getattr(s, f) for f in DiffStats.FIELDS[1:]})
        r.ranges = out[:n].cpu().numpy().view(np.uint64).reshape(n, 2)
        return r

    # -- content-aligned delta ----------------------------------------------------------
    def delta_device(self, a, b, flags, d_ops, cap, stats=None, stream=None):
        """cdc_files_delta_device, raw: d_ops is a device pointer to cap
        cdc_delta_op_t, stats a _lib.cdc_delta_stats_t or None.  Returns the
        number of ops; nothing is written when it exceeds cap."""
        return check(lib().cdc_files_delta_device(a._fh, b._fh, int(flags), _ptr(d_ops), int(cap),
                                                  ctypes.byref(stats) if stats is not None else None, _ptr(stream)))

    def _read_ranges(self, handle, ranges, out):
        """One batch range read: (offset, length, position in `out`) each."""
        reqs = [(handle, o, n, out.data_ptr() + at) for o, n, at in ranges if n]
        if reqs:
            import torch
            torch.cuda.synchronize(out.device)
            assert self.pread_batch_device(reqs) == [r[2] for r in reqs]

    def delta(self, a, b, tables_only=False, literals=False, stream=None):
        """The edit script that builds the file behind `b` (new) out of the one
        behind `a` (old), aligned by content: DeltaStats, whose .ops is the (n, 3)
        uint64 array of (b_off, len, a_off) tiling [0, size_b) -- COPY ops name
        equal bytes of A, LITERAL ops (a_off == DeltaStats.LITERAL) bytes only B
        has.  The span tables give the alignment; a few kilobytes around each
        edit are read for the exact edges.  tables_only: no data is read and
        whole unmatched spans are LITERAL.  literals: .literals holds the LITERAL
        bytes in op order, what a receiver needs besides .ops (apply_delta)."""
        import torch
        dev = f"cuda:{self.device}"
        flags = _lib.CDC_DELTA_TABLES_ONLY if tables_only else 0
        s = _lib.cdc_delta_stats_t()
        cap = 1024
        while True:
            out = torch.empty((cap, 3), dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            n = self.delta_device(a, b, flags, out.data_ptr(), cap, s, stream)
            if n <= cap:
                break
            cap = n  # the exact count: the files cannot change in between
        r = DeltaStats(n_ops=s.ops, **{f: getattr(s, f) for f in DeltaStats.FIELDS[1:]})
        r.ops = out[:n].cpu().numpy().view(np.uint64).reshape(n, 3)
        if literals:
            lit = r.ops[r.ops[:, 2] == DeltaStats.LITERAL]
            at = np.concatenate([[0], np.cumsum(lit[:, 1])]).astype(np.uint64)
            r.literals = torch.empty(int(at[-1]), dtype=torch.uint8, device=dev)
            self._read_ranges(b, [(int(o), int(ln), int(p)) for (o, ln, _), p in zip(lit, at)], r.literals)
        return r

    def apply_delta(self, a, ops, literals):
        """The receiver's half: B's bytes as a CUDA uint8 tensor, from the file
        behind `a`, the ops of a delta and its LITERAL bytes in op order.  The
        COPY ranges of A are read into place in one batch; the literals are
        sliced in."""
        import torch
        dev = f"cuda:{self.device}"
        ops = np.asarray(ops, dtype=np.uint64).reshape(-1, 3)
        size = int(ops[:, 1].sum())
        out = torch.empty(size, dtype=torch.uint8, device=dev)
        lits = torch.as_tensor(literals, dtype=torch.uint8).to(dev) if literals is not None else None
        at = 0
        for b_off, ln, a_off in ops.tolist():
            if a_off == DeltaStats.LITERAL:
                out[b_off:b_off + ln] = lits[at:at + ln]
                at += ln
        self._read_ranges(a, [(a_off, ln, b_off) for b_off, ln, a_off in ops.tolist()
                              if a_off != DeltaStats.LITERAL], out)
        torch.cuda.synchronize(dev)
        return out

    # -- packs: send and receive ----------------------------------------------------------
    def pack_device(self, handle, since, d_have, d_pack, cap, stats=None, stream=None):
        """cdc_file_pack_device, raw: d_have / d_pack are device pointers (or
        None), stats a _lib.cdc_pack_stats_t or None.  Returns total_bytes;
        nothing is written when it exceeds cap."""
        return check(lib().cdc_file_pack_device(handle._fh, since._fh if since is not None else None, _ptr(d_have),
                                                _ptr(d_pack), int(cap),
                                                ctypes.byref(stats) if stats is not None else None, _ptr(stream)))

    def unpack_device(self, name, d_pack, length, hasher=None, flags=0, stats=None, stream=None):
        """cdc_files_unpack_device, raw: d_pack is a device pointer to `length`
        bytes, hasher a Chunker or None.  Returns the span count."""
        return check(lib().cdc_files_unpack_device(self._h, name.encode(), _ptr(d_pack), int(length),
                                                   hasher._h if hasher is not None else None, int(flags),
                                                   ctypes.byref(stats) if stats is not None else None, _ptr(stream)))

    def pack(self, handle, since=None, have=None, stream=None):
        """The file behind `handle` as a pack: (uint8 CUDA tensor, PackStats).
        The pack carries the file's distinct chunks in order of first
        occurrence, except those some span of `since` (a handle, typically of
        a clone taken before edits) names, and those of the spans i with
        have[i] != 0 (`have`: the receiver's contains() answer to hashes(), a
        CUDA uint8 tensor or a host array).  Sizes with cap = 0, allocates,
        packs."""
        import torch
        dev = f"cuda:{self.device}"
        d_have = None
        if have is not None:
            if isinstance(have, torch.Tensor):
                d_have = have.to(dev).contiguous().view(torch.uint8).reshape(-1)
            else:
                d_have = torch.from_numpy(np.ascontiguousarray(have).astype(np.uint8).reshape(-1)).to(dev)
            if d_have.numel() != self.stat(handle)["spans"]:
                raise CdcError(_lib.CDC_EINVAL, "pack: `have` needs one entry per span of the file")
        hp = d_have.data_ptr() if d_have is not None and d_have.numel() else None
        if stream is None:
            torch.cuda.synchronize(dev)
        s = _lib.cdc_pack_stats_t()
        need = self.pack_device(handle, since, hp, None, 0, s, stream)
        out = torch.empty(need, dtype=torch.uint8, device=dev)  # torch allocations are 512-byte aligned
        torch.cuda.synchronize(dev)
        assert self.pack_device(handle, since, hp, out.data_ptr(), need, s, stream) == need
        return out, PackStats._of(s)

    def unpack(self, name, pack, hasher=None, trust=False, stream=None):
        """cdc_files_unpack_device: creates the file `name` from a pack and
        returns PackStats.  `pack` is a CUDA uint8 tensor on this device, one on
        another device, or host bytes / a numpy array (the last two are copied
        over).  `hasher`: any Chunker on this device, for the check of the
        carried chunks' digests (with the store's hasher; a pack made by a
        store with another hasher fails the 'flags' check); trust=True skips the check (a corrupted data byte
        is then stored as it is) and needs no hasher.  The pack is validated
        before anything is written: CdcError(CDC_EINVAL) names the failed
        check, CDC_ENOTFOUND an external span whose chunk this store lacks,
        CDC_EEXIST an existing name, CDC_ENOMEM a store that is too small."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        if isinstance(pack, torch.Tensor):
            t = pack.contiguous().view(torch.uint8).reshape(-1)
            if t.device != dev:
                t = t.to(dev)
        else:
            _, _, arr = _as_buffer(pack)
            t = torch.from_numpy(arr.copy()).to(dev)
        if t.data_ptr() % 16:  # a slice of a larger tensor
            t = t.clone()
        if stream is None:
            torch.cuda.synchronize(dev)
        s = _lib.cdc_pack_stats_t()
        self.unpack_device(name, t.data_ptr() if t.numel() else None, t.numel(), hasher,
                           _lib.CDC_UNPACK_TRUST if trust else 0, s, stream)
        return PackStats._of(s)

    def send(self, handle, to, name=None, since=None, hasher=None):
        """Replicates the file behind `handle` into the FileSystem `to` (on this
        device or another), moving only the chunks `to` lacks: hashes ->
        to.store.contains -> pack(have=...) -> to.unpack.  `name`: the file's
        name there (default: its name here); `since` also excludes what a base
        version names; `hasher`: a Chunker on `to`'s device (None: the carried
        chunks are trusted).  Returns (PackStats of the pack, PackStats of the
        unpack)."""
        import torch
        if self.store.hash != to.store.hash:  # (what the unpack would answer, before anything is packed)
            raise _lib.CdcError(_lib.CDC_EINVAL, f"send: the pack fails the check 'flags': this store hashes with "
                                                 f"{self.store.hash}, the receiving store with {to.store.hash}")
        digests = self.hashes(handle)
        n = digests.shape[0]
        have = np.zeros(n, dtype=np.uint8)
        if n:
            tdev = f"cuda:{to.device}"
            d = torch.from_numpy(np.ascontiguousarray(digests)).to(tdev)
            found = torch.empty(n, dtype=torch.uint8, device=tdev)
            torch.cuda.synchronize(tdev)
            to.store.contains_device(d.data_ptr(), n, found.data_ptr())
            have = found.cpu().numpy()
        pack, sent = self.pack(handle, since=since, have=have)
        got = to.unpack(name if name is not None else handle.name(), pack, hasher=hasher, trust=hasher is None)
        return sent, got

    def save_file(self, handle, path):
        """The file's full pack through host memory into `path` (fails if the
        path exists, as write_file_to_disk).  Returns PackStats."""
        pack, st = self.pack(handle)
        with open(path, "xb") as f:
            pack.cpu().numpy().tofile(f)
        return st

    def load_file(self, name, path, hasher=None, trust=False):
        """unpack() of a pack that save_file wrote."""
        return self.unpack(name, np.fromfile(path, dtype=np.uint8), hasher=hasher, trust=trust)

    # -- reads ----------------------------------------------------------------------
    def read_complete_device(self, handle, d_out, out_cap, d_spans=None, stream=None):
        return check(lib().cdc_file_read_complete_device(handle._fh, _ptr(d_out), out_cap, _ptr(d_spans),
                                                         _ptr(stream)))

    def read_device(self, handle, d_out, out_cap, stream=None):
        return check(lib().cdc_file_read_device(handle._fh, _ptr(d_out), out_cap, _ptr(stream)))

    def pread_device(self, handle, offset, length, d_out, stream=None):
        return check(lib().cdc_file_pread_device(handle._fh, offset, length, _ptr(d_out), _ptr(stream)))

    def pread_batch_device(self, requests, stream=None):
        """cdc_files_pread_batch_device: requests = [(handle, offset, length,
        device pointer)]; returns the byte count of each."""
        n = len(requests)
        reqs = (_lib.cdc_pread_t * max(n, 1))()
        for i, (h, off, ln, dst) in enumerate(requests):
            reqs[i].fh, reqs[i].offset, reqs[i].len, reqs[i].d_dst = h._fh.value, int(off), int(ln), int(dst)
        got = (ctypes.c_uint64 * max(n, 1))()
        check(lib().cdc_files_pread_batch_device(self._h, n, reqs, got, _ptr(stream)))
        return [int(got[i]) for i in range(n)]

    def _to_host(self, fn, cap):
        import torch
        dev = f"cuda:{self.device}"
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        got = fn(out.data_ptr(), cap)
        assert got <= cap
        return out[:got].cpu().numpy()

    def read_file_complete(self, handle):
        """FileSystem::read_file_complete (mod.rs:149-152) as a host uint8 array."""
        size = self.stat(handle)["size"]
        return self._to_host(lambda p, cap: self.read_complete_device(handle, p, cap), size)

    def read_from_file(self, handle):
        """FileSystem::read_from_file (mod.rs:157-160): at most one segment of
        whole spans from the handle's cursor; empty at the end of the file."""
        st = self.stat(handle)
        return self._to_host(lambda p, cap: self.read_device(handle, p, cap), min(self.seg_size, st["size"]))

    def pread(self, handle, offset, length):
        """The bytes [offset, min(offset + length, size)) of the file."""
        size = self.stat(handle)["size"]
        cap = max(0, min(int(length), size - int(offset)))
        return self._to_host(lambda p, _cap: self.pread_device(handle, offset, length if cap else 0, p), cap)

    def hashes(self, handle):
        """FileLayer::read_complete (file_layer.rs:127-133): the (n, 32) span digests."""
        import torch
        n = self.stat(handle)["spans"]
        out = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=f"cuda:{self.device}")
        torch.cuda.synchronize(out.device)
        assert check(lib().cdc_file_hashes_device(handle._fh, _ptr(out.data_ptr()), n)) == n
        return out[:n].cpu().numpy()

    def chunk_count_distribution(self, handle):
        """FileSystem::chunk_count_distribution (mod.rs:166-168): digest bytes ->
        (count, length), in order of first occurrence; the file's last span is
        left out, as file_layer.rs:193-197 does."""
        import torch
        dev = f"cuda:{self.device}"
        cap = max(self.stat(handle)["spans"], 1)
        dig = torch.empty((cap, 32), dtype=torch.uint8, device=dev)
        cnt = torch.empty(cap, dtype=torch.int32, device=dev)
        ln = torch.empty(cap, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        k = check(lib().cdc_file_distribution_device(handle._fh, _ptr(dig.data_ptr()), _ptr(cnt.data_ptr()),
                                                     _ptr(ln.data_ptr()), cap, None))
        dig, cnt, ln = dig[:k].cpu().numpy(), cnt[:k].cpu().numpy(), ln[:k].cpu().numpy()
        return {dig[i].tobytes(): (int(cnt[i]), int(ln[i])) for i in range(k)}

    def get_to_dedup_ratio(self, name, dedup_ratio, stream=None):
        """FileSystem::get_to_dedup_ratio (mod.rs:170-178, file_layer.rs:208-268):
        derives the file "{name}.{ratio:.2}" from the unique spans of `name`,
        repeating the first ceil(U / ratio) of them until the file holds about
        ratio times its unique bytes; returns the new name.  Span offsets in the
        new file are true byte positions (the layer's one deviation).
        CdcError(CDC_EINVAL) for a ratio < 1, NaN or infinite, and when the
        repeating spans are all empty (the reference would not return)."""
        buf = ctypes.create_string_buffer(len(name.encode()) + 400)
        need = check(lib().cdc_files_get_to_dedup_ratio(self._h, name.encode(), float(dedup_ratio), buf, len(buf),
                                                        _ptr(stream)))
        assert need <= len(buf)
        return buf.value.decode()

    def verify_device(self, handle, d_ptr, length, stream=None):
        """cdc_file_verify_device: compares the file with the `length` bytes at
        the device pointer `d_ptr` without reading it back.  Returns (equal,
        first_diff): first_diff is None when equal, else the smallest differing
        byte offset (min(size, length) when only the sizes differ)."""
        diff = ctypes.c_uint64(0)
        same = check(lib().cdc_file_verify_device(handle._fh, _ptr(d_ptr), int(length), ctypes.byref(diff),
                                                  _ptr(stream)))
        return bool(same), (None if same else int(diff.value))

    def write_file_to_disk(self, name, path):
        """FileSystem::write_file_to_disk (mod.rs:181-200): loops read_from_file;
        fails if the path exists."""
        handle = self.open_file_readonly(name)
        with open(path, "xb") as f:
            while True:
                data = self.read_from_file(handle)
                if data.size == 0:
                    break
                f.write(data.tobytes())
        handle._close()

    # -- storage statistics (storage.rs:193-231) ---------------------------------------
    def cdc_dedup_ratio(self):
        return self.store.stats()["cdc_dedup_ratio"]

    def full_cdc_dedup_ratio(self):
        """size_written / (unique bytes + 32 bytes of key per unique digest)."""
        s = self.store.stats()
        if getattr(self.store, "_target", None) is not None:
            return _ratio(s["bytes_written"], self.store.scrub_stats()["cdc_bytes"] + 32 * s["unique_chunks"])
        denom = s["unique_bytes"] + 32 * s["unique_chunks"]
        return s["bytes_written"] / denom if denom else float("nan")

    def total_dedup_ratio(self):
        """FileSystem::total_dedup_ratio (mod.rs:289-291): size_written / (bytes
        of the chunk-kind containers + bytes of the target map's values)."""
        x = self.store.scrub_stats()
        return _ratio(self.store.stats()["bytes_written"], x["cdc_bytes"] + x["target_bytes"])

    def storage_iterator(self):
        """FileSystem::storage_iterator (mod.rs:266-269) as a list; see
        ChunkStore.storage_iterator."""
        return self.store.storage_iterator()

    def average_chunk_size(self):
        return self.store.stats()["average_chunk_size"]

    def clear_database(self):
        """FileSystem::clear_database (mod.rs:275-278): no files, an empty store,
        every open handle invalid."""
        check(lib().cdc_files_clear(self._h))

    def clear_file_system(self):
        """FileSystem::clear_file_system (mod.rs:294-297): clear_database and the
        target map."""
        target = getattr(self.store, "_target", None)
        if target is not None:
            target.clear()  # first: the base's clear then adopts the emptied target
        self.clear_database()

    def scrub(self):
        """FileSystem::scrub (mod.rs:245-247): runs the scrubber the file system
        was created with (new_with_scrubber) and returns its ScrubMeasurements.
        A CDC file system has none: ErrorKind::InvalidInput (storage.rs:180-190)."""
        scrubber = getattr(self, "_scrubber", None)
        if scrubber is None:
            raise CdcError(_lib.CDC_EINVAL, "scrub: this file system was created without a scrubber")
        return self.store.scrub(scrubber)


def version():
    return lib().cdc_version().decode()
