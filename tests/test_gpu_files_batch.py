"""cdc_files_write_batch_device on the GPU: many files written by one call must
leave the layer and the store exactly as one cdc_file_write_device per file, in
request order, would.  Every equality test drives a twin FileSystem through
sequential write_to_file and compares everything observable; the digests, span
lengths and bytes are also held against tests/files_model.py over
tests/store_model.py (hashlib digests, the oracle's chunk lists), so the new
code is never compared with itself alone."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import ae_model
import files_model as fm
import oracle
import store_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 1 << 20
FAST = (64, 256, 1024)
SIZES = {"fast": (4096, 8192, 16384), "rabin": (2048, 4096, 8192), "ultra": (4096, 8192, 16384),
         "leap": (4096, 8192, 16384), "seq": (4096, 8192, 16384), "fixed": (4096, 0, 0),
         "ae": (4096, 8192, 16384)}
STORE_FIELDS = ("chunks_written", "bytes_written", "unique_chunks", "unique_bytes", "arena_capacity", "arena_used")


def _code(excinfo):
    return excinfo.value.code


def _store(fs):
    st = fs.store.stats()
    return tuple(st[k] for k in STORE_FIELDS)


def _lengths(algo, data, sizes):
    """Span lengths of one write of `data` alone: the oracle's, or ae_model's."""
    if data.size == 0:
        return []
    if algo == "ae":
        return [int(x) for x in ae_model.chunk_array(data, *sizes)[:, 1]]
    if algo == "fixed":
        return [int(x) for x in oracle.fixed(data.size, sizes[0])[:, 1]]
    if algo == "fast":
        return [int(x) for x in oracle.fastcdc(data, *sizes)[:, 1]]
    return [int(x) for x in oracle.fs_write(algo, data, *sizes)[0]]


def _host(data):
    if hasattr(data, "cpu"):
        return data.cpu().numpy()
    return data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)


class Reader:
    """Everything observable of one file, through buffers allocated once."""

    def __init__(self, nbytes, nspans):
        import torch
        self.out = torch.empty(max(nbytes, 1) + 2 * sm.GUARD, dtype=torch.uint8, device="cuda")
        self.spans = torch.empty((max(nspans, 1), 2), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def file(self, fs, name, distribution=True):
        h = fs.open_file_readonly(name)
        st = fs.stat(h)
        size, n = st["size"], st["spans"]
        import torch
        self.out.fill_(sm.POISON)
        torch.cuda.synchronize()
        got = fs.read_complete_device(h, self.out.data_ptr() + sm.GUARD, size, self.spans.data_ptr())
        assert got == size
        raw = self.out[:size + 2 * sm.GUARD].cpu().numpy()
        assert (raw[:sm.GUARD] == sm.POISON).all() and (raw[sm.GUARD + size:] == sm.POISON).all()
        res = {"size": size, "spans": n, "bytes": raw[sm.GUARD:sm.GUARD + size].tobytes(),
               "table": self.spans[:n].cpu().numpy().view(np.uint64).tolist(),
               "hashes": [bytes(d) for d in fs.hashes(h)]}
        if distribution:
            res["distribution"] = list(fs.chunk_count_distribution(h).items())
        fs.close_file(h)
        return res


class Twin:
    """`batch` takes write_to_files, `loop` the same data through one
    write_to_file per file, `model` the chunk lists the oracle gives."""

    def __init__(self, c, algo="fixed", sizes=(64, 0, 0), max_chunks=1 << 13, arena=4 * MB, scrubber=None):
        self.c, self.algo, self.sizes = c, algo, sizes
        if algo == "fixed":
            self.ch = c.FSChunker(sizes[0])
        elif algo == "fast":
            self.ch = c.FastChunker(c.SizeParams(*sizes))
        elif algo == "seq":
            self.ch = c.SeqChunker(c.OperationMode.Increasing, c.SizeParams(*sizes))
        else:
            cls = {"rabin": c.RabinChunker, "ultra": c.UltraChunker, "leap": c.LeapChunker, "ae": c.AeChunker}[algo]
            self.ch = cls(c.SizeParams(*sizes))
        if scrubber is None:
            make = lambda: c.FileSystem(max_chunks=max_chunks, arena_bytes=arena)  # noqa: E731
        else:
            make = lambda: c.FileSystem.new_with_scrubber(  # noqa: E731
                scrubber(), max_chunks=max_chunks, arena_bytes=arena, target_max_chunks=max_chunks,
                target_arena_bytes=arena)
        self.batch, self.loop = make(), make()
        self.model = fm.Files()
        self.names = []
        self.bytes = {}

    def _handles(self, fs, names):
        return [fs.open_file(n, self.ch) if fs.file_exists(n) else fs.create_file(n, self.ch) for n in names]

    def write(self, names, datas, stream=None):
        """One batch on `batch`, a loop on `loop`, the oracle's chunks into the model; returns the span counts."""
        bh = self._handles(self.batch, names)
        got = self.batch.write_to_files(bh, datas, stream=stream)
        want = []
        for name, data, h in zip(names, datas, self._handles(self.loop, names)):
            host = _host(data)
            want.append(self.loop.write_to_file(h, host))
            self.loop.close_file(h)
            mh = self.model.open(name) if self.model.exists(name) else self.model.create(name)
            self.model.append_lengths(mh, host, _lengths(self.algo, host, self.sizes))
            if name not in self.bytes:
                self.names.append(name)
            self.bytes[name] = self.bytes.get(name, b"") + host.tobytes()
        assert got == want
        return got, bh

    def compare(self, every=1, model=True):
        """All observables of every file and of the store: batch == loop, and both == the model."""
        assert _store(self.batch) == _store(self.loop)
        if model:
            sm.assert_stats(self.batch.store, self.model.store)
        assert self.batch.list_files() == self.loop.list_files() == self.model.list()
        nbytes = max([len(b) for b in self.bytes.values()] + [1])
        nspans = max([len(s) for s in self.model.files.values()] + [1])
        rd = Reader(nbytes, nspans)
        for k, name in enumerate(self.names):
            dist = k % every == 0
            a, b = rd.file(self.batch, name, dist), rd.file(self.loop, name, dist)
            assert a == b, name
            mh = self.model.open(name)
            spans = self.model._spans(mh)
            assert a["bytes"] == self.bytes[name], name
            assert a["table"] == [[s.offset, s.len] for s in spans], name
            assert a["hashes"] == [s.hash for s in spans], name
            assert (a["size"], a["spans"]) == (len(self.bytes[name]), len(spans))
            if dist:
                assert a["distribution"] == list(self.model.distribution(mh).items()), name


def _random(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8)


# ---- 1. file boundaries inside a wave -----------------------------------------------------------
def test_file_boundaries_inside_a_wave():
    """About 200 files of 0 to 65 spans of 64 bytes: most waves of the length
    pass hold spans of several files; empty files first, last and in runs of three."""
    import chunkfs_amd as c
    rng = np.random.default_rng(101)
    cycle = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 4097]
    lengths = list(itertools.islice(itertools.cycle(cycle), 190))
    for at in (150, 57):
        lengths[at:at] = [0, 0, 0]
    lengths.append(0)
    assert lengths[0] == 0 and lengths[-1] == 0 and lengths[57:60] == [0, 0, 0] and len(lengths) == 197
    t = Twin(c)
    names = [f"f{i:03d}" for i in range(len(lengths))]
    got, _ = t.write(names, [_random(rng, n) for n in lengths])
    assert got == [-(-n // 64) for n in lengths]
    t.compare()


# ---- 2. scan-block edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_scan_block_edges(order):
    """kScanBlockItems = 2048: files whose spans end one short of a scan block,
    straddle it, and start one past the next."""
    import chunkfs_amd as c
    rng = np.random.default_rng(103)
    spans = [2047, 2, 2049, 1]
    if order == "reverse":
        spans.reverse()
    t = Twin(c)
    datas = [_random(rng, n * 64 - 5) for n in spans]
    got, _ = t.write([f"s{i}" for i in range(4)], datas)
    assert got == spans
    t.compare()


# ---- 3. more files than one block of the per-file pass ------------------------------------------------
def test_more_files_than_one_block_and_the_table_pool():
    import chunkfs_amd as c
    rng = np.random.default_rng(107)
    datas = []
    for i in range(1025):
        d = _random(rng, 280 + i % 41)
        if i % 2 == 1:
            d[:128] = datas[i - 1][:128]  # neighbours share a prefix of two chunks
        if i and i % 7 == 0:
            d = datas[0].copy()
        datas.append(d)
    t = Twin(c)
    got, _ = t.write([f"n{i:04d}" for i in range(1025)], datas)
    assert got == [-(-d.size // 64) for d in datas]
    blocks = c._lib.lib().cdc_debug_files_table_blocks(t.batch._h)
    assert 1 <= blocks <= 1025 // 16, blocks
    assert 1 <= c._lib.lib().cdc_debug_files_table_blocks(t.loop._h) <= 1025 // 16
    st = t.batch.store.stats()
    assert st["unique_chunks"] < st["chunks_written"] - 2 * 146  # the copies of file 0 and the shared prefixes
    t.compare(every=16)


# ---- 4. files that already hold spans --------------------------------------------------------------------
def test_files_that_already_hold_spans():
    """63, 64 and 65 spans sit at the 64-span capacity edge; they receive 1, 0
    and 130 more (the last one grows twice over) beside a fresh file."""
    import chunkfs_amd as c
    rng = np.random.default_rng(109)
    t = Twin(c)
    names = ["h63", "h64", "h65"]
    for name, n in zip(names, (63, 64, 65)):  # one write each, through the batch call too
        got, _ = t.write([name], [_random(rng, n * 64)])
        assert got == [n]
    got, handles = t.write(names + ["fresh"], [_random(rng, 10), _random(rng, 0), _random(rng, 130 * 64 - 3),
                                               _random(rng, 200)])
    assert got == [1, 0, 130, 4]
    assert [t.batch.stat(h)["spans"] for h in handles] == [64, 64, 195, 4]
    assert [t.batch.stat(h)["size"] for h in handles] == [63 * 64 + 10, 64 * 64, 65 * 64 + 130 * 64 - 3, 200]
    t.compare()
    table = Reader(200 * 64, 200).file(t.batch, "h65")["table"]
    assert table[65] == [65 * 64, 64] and table[-1] == [194 * 64, 61]  # the offsets continue from the file's size


# ---- 5. dedup order ----------------------------------------------------------------------------------------
def test_dedup_order_is_request_order():
    import chunkfs_amd as c
    rng = np.random.default_rng(113)
    a, b, cc, d, e = (_random(rng, 64) for _ in range(5))
    x = np.concatenate([a, b, a, cc, a, b[:40]])
    y = np.concatenate([d, b, e, a[:7]])
    t = Twin(c, max_chunks=256, arena=64 << 10)
    got, _ = t.write(["x", "y", "x-again"], [x, y, x])
    assert got == [6, 4, 6]
    st = t.batch.store.stats()
    assert (st["chunks_written"], st["unique_chunks"]) == (16, 7)
    assert t.batch.store.storage_iterator() == t.loop.store.storage_iterator()
    t.compare()
    got, _ = t.write(["x", "y", "x-again"], [x, y, x])  # the same data again: appended, nothing new stored
    assert got == [6, 4, 6]
    st = t.batch.store.stats()
    assert (st["chunks_written"], st["unique_chunks"]) == (32, 7)
    assert t.batch.store.storage_iterator() == t.loop.store.storage_iterator()
    t.compare()


# ---- 6. every chunker ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["fast", "fixed", "rabin", "ultra", "leap", "seq", "ae"])
def test_every_chunker_sees_each_request_as_its_own_buffer(algo):
    import chunkfs_amd as c
    sizes = [0, 10, 4096, 70001, 150000, 300 << 10, 33333, 200001]
    datas = [oracle.splitmix64_bytes(n, 700 + i) for i, n in enumerate(sizes)]
    t = Twin(c, algo, SIZES[algo], max_chunks=1 << 11, arena=3 * MB)
    got, _ = t.write([f"{algo}{i}" for i in range(len(sizes))], datas)
    want = [len(_lengths(algo, d, SIZES[algo])) for d in datas]
    assert got == want and want[0] == 0 and want[1] == 1
    t.compare()


# ---- 7. refusals change nothing ------------------------------------------------------------------------------------
def _snapshot(fs, names):
    out = [_store(fs)]
    for name in names:
        h = fs.open_file_readonly(name)
        st = fs.stat(h)
        out.append((name, st["size"], st["spans"], fs.hashes(h).tobytes()))
        fs.close_file(h)
    return out


def _call(c, fs, ch, reqs):
    """The C entry point on (handle, device pointer, length) requests: (return value, span counts)."""
    arr = (c._lib.cdc_fwrite_t * len(reqs))()
    for i, (h, ptr, n) in enumerate(reqs):
        arr[i].fh, arr[i].d_data, arr[i].len = h._fh.value, ptr, n
    spans = (ctypes.c_uint64 * len(reqs))(*([77] * len(reqs)))
    rc = c._lib.lib().cdc_files_write_batch_device(fs._h, ch._h, len(reqs), arr, spans, None)
    return rc, list(spans)


def test_refusals_change_nothing():
    import chunkfs_amd as c
    E = c._lib
    rng = np.random.default_rng(127)
    ch = c.FSChunker(64)
    fs = c.FileSystem(max_chunks=128, arena_bytes=4096)
    other = c.FileSystem(max_chunks=128, arena_bytes=4096)
    names = ["a", "b", "c"]
    hs = [fs.create_file(n, ch) for n in names]
    assert fs.write_to_files(hs, [_random(rng, 200), _random(rng, 64), _random(rng, 300)]) == [4, 1, 5]
    before = _snapshot(fs, names)
    buf = sm.dev(_random(rng, 8192))
    ones = sm.dev(np.arange(130 * 16, dtype=np.uint8))  # 130 distinct one-byte files at 16-byte steps
    p = buf.data_ptr()

    def refused(rc_spans, code, words=None):
        rc, spans = rc_spans
        assert rc == code, (rc, E.lib().cdc_last_error())
        assert words is None or words in E.lib().cdc_last_error().decode()
        assert spans == [77] * len(spans)
        assert _snapshot(fs, names) == before

    ro = fs.open_file_readonly("b")
    refused(_call(c, fs, ch, [(hs[0], p, 64), (ro, p, 64), (hs[2], p, 64)]), E.CDC_EPERM)
    with pytest.raises(c.CdcError) as ei:  # the Python mirror refuses before it touches the data
        fs.write_to_files([hs[0], ro, hs[2]], [object(), object(), object()])
    assert _code(ei) == E.CDC_EPERM and _snapshot(fs, names) == before
    twice = fs.open_file("a", ch)
    refused(_call(c, fs, ch, [(hs[0], p, 64), (hs[1], p, 64), (twice, p + 64, 64)]), E.CDC_EINVAL, "twice")
    foreign = other.create_file("a", ch)
    refused(_call(c, fs, ch, [(hs[0], p, 64), (foreign, p, 64)]), E.CDC_EINVAL, "another layer")
    refused(_call(c, fs, ch, [(hs[0], p, 64), (hs[1], None, 64)]), E.CDC_EINVAL, "NULL data")
    extra = [fs.create_file(f"x{i:03d}", ch) for i in range(130)]
    names += [f"x{i:03d}" for i in range(130)]
    before = _snapshot(fs, names)
    # 130 one-byte chunks fit the arena (16 bytes each) but not max_chunks = 128 beside the 10 stored
    refused(_call(c, fs, ch, [(h, ones.data_ptr() + 16 * i, 1) for i, h in enumerate(extra)]), E.CDC_ENOMEM,
            "max_chunks")
    # 100 chunks of 64 bytes fit max_chunks but not the 4096-byte arena
    refused(_call(c, fs, ch, [(hs[0], p, 50 * 64), (hs[1], p + 50 * 64, 50 * 64)]), E.CDC_ENOMEM, "arena")
    rc, spans = _call(c, fs, ch, [(hs[0], p, 64), (hs[1], None, 0), (hs[2], p + 64, 100)])  # one that fits is taken
    assert (rc, spans) == (3, [1, 0, 2])
    fs.store.clear()
    before = _snapshot(fs, names)
    refused(_call(c, fs, ch, [(extra[0], p, 64), (hs[1], p, 64)]), E.CDC_ENOTFOUND, "cleared")
    rc, spans = _call(c, fs, ch, [(extra[0], p, 64), (extra[1], p, 64)])  # files without spans may be written
    assert (rc, spans) == (2, [1, 1]) and fs.store.stats()["unique_chunks"] == 1


# ---- 8. scrubbed state ---------------------------------------------------------------------------------------------
def test_batch_in_the_scrubbed_state():
    import chunkfs_amd as c
    rng = np.random.default_rng(131)
    t = Twin(c, "fast", FAST, max_chunks=1 << 11, arena=MB, scrubber=c.CopyScrubber)
    old = [_random(rng, 20000), _random(rng, 7000)]
    t.write(["o0", "o1"], old)
    for fs in (t.batch, t.loop):
        assert fs.scrub().processed_data > 0
        assert fs.store.scrub_stats()["chunk_containers"] == 0
    mixed = [np.concatenate([_random(rng, 3000), old[0][:12000]]), old[1].copy(), _random(rng, 5000),
             np.concatenate([old[1], _random(rng, 900)])]
    got, _ = t.write(["m0", "m1", "m2", "o0"], mixed)
    assert all(n > 1 for n in got)
    assert t.batch.store.scrub_stats() == t.loop.store.scrub_stats()
    assert t.batch.store.storage_iterator() == t.loop.store.storage_iterator()
    assert t.batch.target.stats() == t.loop.target.stats()
    t.compare(model=False)  # the model has no target map; the bytes, spans and digests are still the oracle's


# ---- 9. stream order ---------------------------------------------------------------------------------------------------
def test_stream_order_on_a_user_stream():
    """The inputs are produced on a user stream right before the batch, which is
    submitted on that stream with no host wait in between."""
    import torch
    import chunkfs_amd as c
    E = c._lib
    sizes = [300000, 0, 64 << 10, 100001]
    fs = c.FileSystem(max_chunks=1 << 10, arena_bytes=2 * MB)
    ch = c.FastChunker(c.SizeParams(4096, 8192, 16384))
    hs = [fs.create_file(f"s{i}", ch) for i in range(len(sizes))]
    src = [torch.zeros(max(n, 16), dtype=torch.uint8, device="cuda") for n in sizes]
    bufs = [torch.zeros(max(n, 16), dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for i, n in enumerate(sizes):
        if n:
            E.check(E.lib().cdc_fill_splitmix64_device(ctypes.c_void_p(src[i].data_ptr()), n, 900 + i,
                                                      ctypes.c_void_p(s.cuda_stream)))
    with torch.cuda.stream(s):
        for _ in range(20):  # keep the stream busy ahead of the copies the batch depends on
            bufs[0].add_(1)
        for b, x in zip(bufs, src):
            b.copy_(x)
    got = fs.write_to_files(hs, [b[:n] for b, n in zip(bufs, sizes)], stream=s.cuda_stream)
    for i, n in enumerate(sizes):
        data = oracle.splitmix64_bytes(n, 900 + i)
        assert got[i] == (len(oracle.fastcdc(data, 4096, 8192, 16384)) if n else 0)
        assert (fs.read_file_complete(hs[i]) == data).all()


# ---- 10. timing shares -----------------------------------------------------------------------------------------------------
def test_timing_is_shared_by_length():
    import chunkfs_amd as c
    rng = np.random.default_rng(137)
    fs = c.FileSystem(max_chunks=1 << 10, arena_bytes=MB)
    ch = c.FastChunker(c.SizeParams(*FAST))
    hs = [fs.create_file(f"t{i}", ch) for i in range(3)]
    fs.write_to_files(hs, [_random(rng, 30000), _random(rng, 0), _random(rng, 10000)])
    st = [fs.stat(h) for h in hs]
    assert sum(x["chunk_seconds"] for x in st) > 0 and sum(x["hash_seconds"] for x in st) > 0
    assert st[1]["chunk_seconds"] == 0 and st[1]["hash_seconds"] == 0
    for key in ("chunk_seconds", "hash_seconds"):  # 30000 : 10000 bytes
        assert st[0][key] == pytest.approx(3 * st[2][key], rel=1e-9)


# ---- 11. Python and fixture ---------------------------------------------------------------------------------------------------
def test_python_mixes_host_bytes_and_cuda_tensors():
    import torch
    import chunkfs_amd as c
    from chunkfs_amd import bench
    rng = np.random.default_rng(139)
    raw = [_random(rng, n) for n in (5000, 17, 0, 33000, 1, 4096)]
    big = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), raw[3]])).cuda()
    datas = [raw[0].tobytes(), torch.from_numpy(raw[1]).cuda(), b"", big[3:],  # a tensor view off 16-byte alignment
             bytearray(raw[4].tobytes()), raw[5]]
    t = Twin(c, "fast", FAST, max_chunks=1 << 10, arena=MB)
    t.write([f"p{i}" for i in range(6)], datas)
    t.compare()
    assert t.batch.write_to_files([], []) == []
    with pytest.raises(ValueError):
        t.batch.write_to_files([t.batch.create_file("lonely", t.ch)], [])

    fx = bench.CDCFixture(max_chunks=1 << 10, arena_bytes=MB)
    names = fx.fill_with_many(datas, t.ch)
    assert len(set(names)) == 6 and sorted(names) == fx.fs.list_files()
    for name, want in zip(names, raw):
        assert (fx.fs.read_file_complete(fx.fs.open_file_readonly(name)) == want).all()
    assert _store(fx.fs) == _store(t.loop)


# ---- 12. the C++ mirror ------------------------------------------------------------------------------------------------------------
def test_cpp_files_batch_mirror_runs():
    from chunkfs_amd import _lib, build
    exe = os.path.join(ROOT, "_build", "files_batch_example")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "examples", "files_batch_example.cpp"),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd", "-L", os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
                    "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch ok: 4 files," in r.stdout
