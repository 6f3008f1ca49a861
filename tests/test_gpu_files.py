"""Device file layer (include/chunkfs_amd.h "File layer") on the GPU, through
the C ABI's Python mirror, bit-exact against tests/files_model.py: the
reference's FileLayer / FileSystem semantics (src/system/file_layer.rs,
src/system/mod.rs) with true span offsets.  Every output buffer is guarded by
poisoned bytes (store_model.Guarded)."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import files_model as fm
import oracle
import store_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "filesystem_known_answers.json")))
MB = 1 << 20
SIZES = {"fast": (4096, 8192, 16384), "rabin": (2048, 4096, 8192), "ultra": (4096, 8192, 16384),
         "leap": (4096, 8192, 16384), "seq": (4096, 8192, 16384), "fixed": (4096, 0, 0)}


def _code(excinfo):
    return excinfo.value.code


def _chunker(c, algo, sizes=None):
    s = sizes or SIZES[algo]
    if algo == "fixed":
        return c.FSChunker(s[0])
    if algo == "seq":
        return c.SeqChunker(c.OperationMode.Increasing, c.SizeParams(*s))
    cls = {"fast": c.FastChunker, "rabin": c.RabinChunker, "ultra": c.UltraChunker, "leap": c.LeapChunker}[algo]
    return cls(c.SizeParams(*s))


def _tiling(lengths):
    lengths = np.asarray(lengths, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64) if len(lengths) else lengths
    return np.stack([offs, lengths], axis=1)


def _digests(data, chunks):
    return np.array([np.frombuffer(hashlib.sha256(data[int(o):int(o) + int(ln)].tobytes()).digest(), dtype=np.uint8)
                     for o, ln in chunks], dtype=np.uint8).reshape(-1, 32)


class Pair:
    """The device layer and the model, driven side by side."""

    def __init__(self, c, seg=fm.SEG_SIZE, max_chunks=1 << 12, arena=8 * MB):
        self.c = c
        self.fs = c.FileSystem(max_chunks=max_chunks, arena_bytes=arena, seg_size=seg)
        self.m = fm.Files(seg_size=seg)
        self.seg = seg

    def create(self, name, chunker=None, create_new=True):
        return self.fs.create_file(name, chunker, create_new), self.m.create(name, create_new)

    def open(self, name, chunker=None, readonly=False):
        h = self.fs.open_file_readonly(name) if readonly else self.fs.open_file(name, chunker)
        return h, self.m.open(name, readonly)

    def append(self, hm, data, chunks):
        """cdc_file_append_device of a hand-made chunk list; the model takes the same."""
        h, mh = hm
        chunks = np.asarray(chunks, dtype=np.uint64).reshape(-1, 2)
        d_data = sm.dev(data if data.size else np.zeros(1, dtype=np.uint8))
        dc, dd = sm.dev_chunks(chunks if len(chunks) else np.zeros((1, 2), np.uint64)), sm.dev(_digests(data, chunks))
        got = self.fs.append_device(h, d_data.data_ptr(), data.size, dc.data_ptr(),
                                    dd.data_ptr() if len(chunks) else None, len(chunks))
        assert got == len(chunks)
        self.m.append(mh, data, chunks)

    def write(self, hm, data, lengths):
        """write_to_file (chunk + SHA-256 + put + append on the GPU); the model
        takes the span lengths the oracle gives for the same call."""
        h, mh = hm
        assert self.fs.write_to_file(h, data) == len(lengths)
        self.m.append_lengths(mh, data, lengths)

    def check_file(self, hm, shift=0, stream=None):
        """stat, read_complete with its spans, and the digests, against the model."""
        h, mh = hm
        spans = self.m._spans(mh)
        want = self.m.read_complete(mh)
        st = self.fs.stat(h)
        assert (st["size"], st["spans"]) == (want.size, len(spans))
        g = sm.Guarded(want.size, len(spans), shift)
        got = self.fs.read_complete_device(h, g.out_ptr, want.size, g.spans.data_ptr(), stream)
        assert got == want.size
        a, body, z, sp = g.host()
        assert (a == sm.POISON).all() and (z == sm.POISON).all(), "read_complete wrote outside d_out"
        assert (body == want).all()
        assert sp.tolist() == [[s.offset, s.len] for s in spans]
        dig = self.fs.hashes(h)
        assert [bytes(d) for d in dig] == self.m.hashes(mh)
        return want

    def read_segment(self, hm):
        """One cdc_file_read_device into a guarded segment-sized buffer, against the model's read."""
        h, mh = hm
        want = self.m.read(mh)
        g = sm.Guarded(self.seg, 0)
        got = self.fs.read_device(h, g.out_ptr, self.seg)
        a, body, z, _ = g.host()
        assert got == want.size
        assert (a == sm.POISON).all() and (z == sm.POISON).all() and (body[got:] == sm.POISON).all()
        assert (body[:got] == want).all()
        assert self.fs.stat(h)["cursor"] == mh.offset
        return want

    def pread(self, hm, offset, length, shift=0):
        h, mh = hm
        want = self.m.pread(mh, offset, length)
        g = sm.Guarded(length, 0, shift)
        got = self.fs.pread_device(h, offset, length, g.out_ptr)
        a, body, z, _ = g.host()
        assert got == want.size, (offset, length, got, want.size)
        assert (a == sm.POISON).all() and (z == sm.POISON).all() and (body[got:] == sm.POISON).all()
        assert (body[:got] == want).all(), (offset, length)
        return want


# ---- the reference's file tests (tests/golden/filesystem_known_answers.json) -----------
def _fill(case_writes):
    return [np.full(w["len"], w["byte"], dtype=np.uint8) for w in case_writes]


def test_blocks_read_back_as_four_segments_then_empty():
    import chunkfs_amd as c
    case = KNOWN["write_read_blocks"]
    size = case["chunker"]["size"]
    p = Pair(c, seg=KNOWN["seg_size"])
    w = p.create("file", c.FSChunker(size))
    for data in _fill(case["writes"]):
        p.write(w, data, oracle.fixed(data.size, size)[:, 1])
    assert p.fs.close_file(w[0])["chunk_time"] > 0
    r = p.open("file", c.FSChunker(size))
    got = [p.read_segment(r) for _ in range(case["reads"])]
    assert [g.size for g in got] == case["read_lengths"]
    assert sum(g.size for g in got) == case["total"]
    assert p.read_segment(r).size == case["next_read_length"]
    assert p.fs.stat(r[0])["cursor"] == case["total"]
    host = [p.fs.read_from_file(h2) for h2 in [p.fs.open_file_readonly("file")] for _ in range(2)]
    assert (host[0] == 1).all() and (host[1] == 2).all() and host[0].size == MB


def test_small_file_and_two_handles():
    import chunkfs_amd as c
    case = KNOWN["small_file"]
    p = Pair(c)
    w = p.create("file", c.FSChunker(case["chunker"]["size"]))
    data = _fill(case["writes"])[0]
    p.write(w, data, [data.size])
    r = p.open("file", readonly=case["readonly"])
    assert p.read_segment(r).size == case["read_lengths"][0]
    assert (p.fs.read_file_complete(r[0]) == data).all()

    case = KNOWN["two_handles"]
    h1 = p.create("two", c.FSChunker(4096))
    h2 = p.open("two", readonly=True)  # opened before the write
    data = _fill(case["writes"])[0]
    p.write(h1, data, oracle.fixed(data.size, 4096)[:, 1])
    p.fs.close_file(h1[0])
    assert p.check_file(h2).size == case["read_complete_length"]
    assert sorted(p.fs.list_files()) == p.m.list() == ["file", "two"]
    assert p.fs.file_exists("two") and not p.fs.file_exists("three")


def test_readonly_and_name_rules():
    import chunkfs_amd as c
    case = KNOWN["readonly_rules"]
    p = Pair(c)
    ch = c.FSChunker(case["chunker"]["size"])
    w = p.create("file", ch)
    data = _fill(case["writes"])[0]
    p.write(w, data, oracle.fixed(data.size, 4096)[:, 1])
    p.fs.close_file(w[0])
    ro = p.open("file", readonly=True)
    before, store_before = p.fs.stat(ro[0]), p.fs.store.stats()
    with pytest.raises(c.CdcError) as ei:
        p.fs.write_to_file(ro[0], data)
    assert _code(ei) == c._lib.CDC_EPERM and case["write_error"] == "PermissionDenied"
    d_data, dc, dd = sm.dev(data[:16]), sm.dev_chunks([[0, 16]]), sm.dev(_digests(data, [[0, 16]]))
    with pytest.raises(c.CdcError) as ei:  # the C entry points refuse too
        p.fs.append_device(ro[0], d_data.data_ptr(), 16, dc.data_ptr(), dd.data_ptr(), 1)
    assert _code(ei) == c._lib.CDC_EPERM
    rc = c._lib.lib().cdc_file_write_device(ro[0]._fh, ch._h, ctypes.c_void_p(d_data.data_ptr()), 16, None)
    assert rc == c._lib.CDC_EPERM
    assert p.fs.stat(ro[0]) == before and p.fs.store.stats() == store_before
    got = p.check_file(ro)
    assert got.size == case["read_complete_length"] and (got == case["read_complete_byte"]).all()
    p.read_segment(ro)
    assert p.fs.close_file(ro[0]) == case["close_measurements"]

    with pytest.raises(c.CdcError) as ei:
        p.fs.create_file("file", ch, create_new=False)
    assert _code(ei) == c._lib.CDC_EEXIST
    for opener in (lambda: p.fs.open_file("nope", ch), lambda: p.fs.open_file_readonly("nope")):
        with pytest.raises(c.CdcError) as ei:
            opener()
        assert _code(ei) == c._lib.CDC_ENOTFOUND
    old = p.open("file", readonly=True)
    t = p.create("file", ch, create_new=True)  # truncates; the store keeps its chunks
    assert p.fs.stat(t[0])["size"] == 0 and p.fs.read_file_complete(old[0]).size == 0
    assert p.fs.store.stats() == store_before
    p.write(t, data[:5000], [4096, 904])
    p.check_file(old)
    with pytest.raises(c.CdcError) as ei:
        p.fs.scrub()
    assert _code(ei) == c._lib.CDC_EINVAL


def test_dedup_ratios():
    import chunkfs_amd as c
    case = KNOWN["dedup_ratio_fixed_4096"]
    fs = c.FileSystem(max_chunks=1 << 10, arena_bytes=4 * MB)
    ch = c.FSChunker(case["chunker"]["size"])
    for i, step in enumerate(case["steps"]):
        h = fs.create_file("file", ch) if i == 0 else fs.open_file("file", ch)
        fs.write_to_file(h, np.full(step["len"], step["byte"], dtype=np.uint8))
        fs.close_file(h)
        assert fs.cdc_dedup_ratio() == step["ratio"]
    assert fs.average_chunk_size() == 4096
    assert fs.full_cdc_dedup_ratio() == 3 * MB / (2 * 4096 + 2 * 32)
    h = fs.open_file_readonly("file")  # appended through re-opened handles: true offsets
    assert fs.stat(h)["size"] == 3 * MB
    got = fs.read_file_complete(h)
    assert (got[:2 * MB] == 10).all() and (got[2 * MB:] == 20).all()
    segs = [fs.read_from_file(h).size for _ in range(4)]
    assert segs == [MB, MB, MB, 0]


# ---- segment reads ------------------------------------------------------------------
@pytest.mark.parametrize("algo,sizes", [("fast", (64, 256, 1024)), ("fixed", (512, 0, 0))])
def test_segment_reads_match_the_model(algo, sizes, tmp_path):
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(64 << 10, 99)
    p = Pair(c, seg=4096)
    w = p.create("f", _chunker(c, algo, sizes))
    lengths, _ = oracle.fs_write(algo, data, *sizes)
    p.write(w, data, lengths)
    p.check_file(w)
    r = p.open("f", readonly=True)
    total = 0
    while True:
        got = p.read_segment(r)
        if got.size == 0:
            break
        assert (got == data[total:total + got.size]).all()
        total += got.size
    assert total == data.size and p.fs.stat(r[0])["cursor"] == data.size
    assert p.read_segment(r).size == 0
    out = tmp_path / "f.bin"
    p.fs.write_file_to_disk("f", str(out))
    assert out.read_bytes() == data.tobytes()
    with pytest.raises(FileExistsError):
        p.fs.write_file_to_disk("f", str(out))


def test_hand_made_spans():
    """cdc_file_append_device: a span of exactly the segment, one of segment + 1
    (0 bytes, cursor stuck), length-0 spans at the start, middle and end, and
    chunks that neither tile nor stay apart in the data."""
    import chunkfs_amd as c
    seg = 4096
    rng = np.random.default_rng(17)
    data = rng.integers(0, 256, 20000, dtype=np.uint8)
    p = Pair(c, seg=seg)
    w = p.create("mixed")
    chunks = [[0, 0], [10, seg], [5000, 0], [5000, 100], [4000, 300], [6000, seg + 1], [12000, 50], [12050, 0]]
    p.append(w, data, chunks[:3])
    p.append(w, data, np.zeros((0, 2), dtype=np.uint64))  # an empty append is legal
    p.append(w, data, chunks[3:])
    p.check_file(w, shift=3)
    r = p.open("mixed", readonly=True)
    assert [p.read_segment(r).size for _ in range(4)] == [seg, 400, 0, 0]
    assert r[1].offset == seg + 400 < p.m.size(r[1])  # stuck in front of the long span, as the reference
    for off, ln in [(0, 1), (seg - 1, 2), (seg, 400), (seg + 399, 4099), (0, 20000), (8593, 50), (8642, 5)]:
        p.pread(r, off, ln, shift=off % 16)

    first = p.create("long_first")
    p.append(first, data, [[0, seg + 1], [7, 9]])
    r = p.open("long_first", readonly=True)
    assert p.read_segment(r).size == 0 and p.fs.stat(r[0])["cursor"] == 0
    exact = p.create("exact")
    p.append(exact, data, [[0, 0], [100, seg], [0, 0], [9000, seg], [0, 0]])
    r = p.open("exact", readonly=True)
    assert [p.read_segment(r).size for _ in range(3)] == [seg, seg, 0]
    zeros = p.create("zeros")
    p.append(zeros, data, [[0, 0], [5, 0], [20000, 0]])
    assert p.check_file(zeros).size == 0
    assert p.read_segment(p.open("zeros", readonly=True)).size == 0
    assert p.pread(zeros, 0, 10).size == 0
    assert p.fs.chunk_count_distribution(zeros[0]) == p.m.distribution(zeros[1])


# ---- byte ranges ----------------------------------------------------------------------
def _three_files(c):
    rng = np.random.default_rng(23)
    p = Pair(c, max_chunks=1 << 10, arena=2 * MB)
    handles = []
    for k, n in enumerate((60, 35, 48)):
        lengths = rng.integers(1, 5001, n)
        if k == 2:
            lengths[[0, 7, 8, n - 1]] = 0  # equal offsets inside the searches
        lengths[3] = 5000
        lengths[4] = 1
        data = rng.integers(0, 256, int(lengths.sum()), dtype=np.uint8)
        h = p.create(f"file{k}")
        p.append(h, data, _tiling(lengths))
        handles.append(h)
    return p, handles


def _ranges(p, hm, rng):
    """(offset, length) ranges over one file: mid-chunk starts and ends, inside
    one chunk, exactly one chunk, empty, at and past the end."""
    spans = [s for s in p.m._spans(hm[1]) if s.len]
    size = p.m.size(hm[1])
    out = [(0, 0), (5, 0), (size, 10), (size + 100, 10), (size - 1, 1), (size - 3, 100), (0, size), (0, size + 7),
           (1, size - 2)]
    for s in (spans[1], spans[3], spans[4], spans[-1]):
        out += [(s.offset, s.len), (s.offset, 1), (s.offset + s.len - 1, 1), (s.offset + s.len - 1, 2)]
        if s.len > 2:
            out += [(s.offset + 1, s.len - 2)]
    for _ in range(30):
        a = int(rng.integers(0, size))
        out.append((a, int(rng.integers(1, 20000))))
    return out


def test_pread_sweep_and_batch():
    import torch
    import chunkfs_amd as c
    p, handles = _three_files(c)
    rng = np.random.default_rng(29)
    for hm in handles:
        p.check_file(hm)
    reqs = []
    for k, hm in enumerate(handles):
        r = p.open(f"file{k}", readonly=True)
        for i, (off, ln) in enumerate(_ranges(p, r, rng)):
            p.pread(r, off, ln, shift=(i + 5 * k) % 16)
            reqs.append((r, off, ln))
    f0 = p.open("file0", readonly=True)
    for t in range(16):  # every destination alignment, a range that starts and ends mid-chunk
        p.pread(f0, 777 + t, 9000, shift=t)
        p.pread(f0, 4321, 16 + t, shift=15 - t)

    # pread_batch: all of the above (~200 mixed requests over the three files) in one call
    order = rng.permutation(len(reqs))
    reqs = [reqs[i] for i in order] + [(f0, 777 + t, 9000) for t in range(16)]
    assert 150 <= len(reqs) <= 260
    at, places = sm.GUARD, []
    for i, (_, _, ln) in enumerate(reqs):
        at += (i * 7) % 16  # every alignment
        places.append(at)
        at += ln + 32
    image = np.full(at + sm.GUARD, sm.POISON, dtype=np.uint8)
    buf = torch.full((image.size,), sm.POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    want_counts = []
    for (hm, off, ln), where in zip(reqs, places):
        w = p.m.pread(hm[1], off, ln)
        image[where:where + w.size] = w
        want_counts.append(w.size)
    got = p.fs.pread_batch_device([(hm[0], off, ln, buf.data_ptr() + where)
                                   for (hm, off, ln), where in zip(reqs, places)])
    assert got == want_counts
    assert (buf.cpu().numpy() == image).all()
    assert p.fs.pread_batch_device([]) == []


def test_ranges_that_touch_as_many_spans_as_bytes_allow():
    """The planner sizes its piece list from the file's shortest span and its
    count of length-0 spans: ranges made of shortest spans only, with length-0
    spans between them and a partial span at each end, sit on that bound."""
    import chunkfs_amd as c
    seg = 4096
    rng = np.random.default_rng(53)
    lengths = [100] + [64, 0] * 64 + [100] + [64] * 64 + [0, 0, 3000, 64]
    data = rng.integers(0, 256, sum(lengths), dtype=np.uint8)
    p = Pair(c, seg=seg)
    w = p.create("f")
    cut = 70
    p.append(w, data, _tiling(lengths)[:cut])  # two appends: the statistics accumulate
    rest = _tiling(lengths)[cut:]
    p.append(w, data, rest)
    p.check_file(w)
    r = p.open("f", readonly=True)
    p.pread(r, 50, 50 + 64 * 64 + 50, shift=7)       # partial, 64 shortest + 64 empty, partial
    p.pread(r, 100, 64 * 64)                          # exactly the 64 shortest spans
    p.pread(r, 99, 64 * 64 + 2)
    p.pread(r, 100 + 64 * 64 + 100 - 1, 64 * 64 + 2)  # the run without empty spans, one byte either side
    total = 0
    while True:
        got = p.read_segment(r)
        if got.size == 0:
            break
        total += got.size
    assert total == data.size


# ---- deduplicated file, distribution ----------------------------------------------------
def _versions():
    """A base blob plus three mutated copies (the construction of the store's round-trip test)."""
    rng = np.random.default_rng(3)
    versions = [oracle.splitmix64_bytes(2 << 20, 7)]
    for k in range(3):
        v = versions[-1].copy()
        for _ in range(20):
            q = int(rng.integers(0, v.size - 5000))
            if k % 3 == 0:
                v[q:q + 100] = rng.integers(0, 256, 100, dtype=np.uint8)
            elif k % 3 == 1:
                v = np.concatenate([v[:q], rng.integers(0, 256, 333, dtype=np.uint8), v[q:]])
            else:
                v = np.concatenate([v[:q], v[q + 777:]])
        versions.append(v)
    return versions


def test_deduplicated_file_and_distribution():
    import chunkfs_amd as c
    sizes = SIZES["fast"]
    p = Pair(c, max_chunks=1 << 12, arena=12 * MB)
    w = p.create("versions", c.FastChunker(c.SizeParams(*sizes)))
    whole = []
    for v in _versions():
        p.write(w, v, oracle.fastcdc(v, *sizes)[:, 1])
        whole.append(v)
    rep = whole[0][1000:1777]
    p.append(w, rep, np.array([[0, rep.size]] * 1000, dtype=np.uint64))  # one chunk, 1000 times
    tail = np.frombuffer(b"the last span is left out of the distribution", dtype=np.uint8).copy()
    p.append(w, tail, [[0, tail.size]])
    data = np.concatenate(whole + [np.tile(rep, 1000), tail])
    assert (p.check_file(w) == data).all()
    assert p.fs.cdc_dedup_ratio() > 1.5
    got, want = p.fs.chunk_count_distribution(w[0]), p.m.distribution(w[1])
    assert list(got.items()) == list(want.items())  # first-occurrence order, counts, lengths
    assert got[fm.sha(rep)] == (1000, rep.size)
    assert fm.sha(tail) not in got and max(n for n, _ in got.values()) == 1000
    assert 1 < sum(1 for n, _ in got.values() if n == 4) and len(got) < p.fs.stat(w[0])["spans"] - 1
    # snprintf convention: one entry short writes nothing
    import torch
    k = len(got)
    dig = torch.full((k, 32), sm.POISON, dtype=torch.uint8, device="cuda")
    cnt = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    ln = torch.full((k,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L = c._lib.lib()
    P = ctypes.c_void_p
    assert L.cdc_file_distribution_device(w[0]._fh, P(dig.data_ptr()), P(cnt.data_ptr()), P(ln.data_ptr()), k - 1,
                                          None) == k
    assert (dig.cpu().numpy() == sm.POISON).all() and (cnt.cpu().numpy() == -1).all() and (ln.cpu().numpy() == -1).all()


def test_span_table_growth():
    """300 one-chunk appends to one file, writes to a second in between: the
    table doubles several times, by copies on the call's stream."""
    import chunkfs_amd as c
    rng = np.random.default_rng(31)
    data = rng.integers(0, 256, 64 << 10, dtype=np.uint8)
    p = Pair(c, max_chunks=1 << 11, arena=2 * MB)
    a, b = p.create("a"), p.create("b")
    for i in range(300):
        o, ln = int(rng.integers(0, data.size - 600)), int(rng.integers(0, 600))
        p.append(a, data, [[o, ln]])
        if i % 25 == 0:
            p.append(b, data, [[i, 100], [i + 50, 900], [0, 0]])
    assert p.fs.stat(a[0])["spans"] == 300 and p.fs.stat(b[0])["spans"] == 36
    p.check_file(a)
    p.check_file(b, shift=9)
    size = p.m.size(a[1])
    p.pread(a, size // 3, size // 2, shift=1)


# ---- every chunker through cdc_file_write_device ---------------------------------------------
@pytest.mark.parametrize("algo", ["fast", "fixed", "rabin", "ultra", "leap", "seq"])
def test_every_chunker_writes_and_reads_back(algo):
    import torch
    import chunkfs_amd as c
    ch = _chunker(c, algo)
    fs = c.FileSystem(max_chunks=1 << 11, arena_bytes=3 * MB)
    for name, data in (("zeros", np.zeros(MB, dtype=np.uint8)), ("random", oracle.splitmix64_bytes(MB, 1234))):
        want, _ = oracle.fs_write(algo, data, *SIZES[algo])
        h = fs.create_file(name, ch)
        assert fs.write_to_file(h, data) == len(want)
        g = sm.Guarded(data.size, len(want))
        assert fs.read_complete_device(h, g.out_ptr, data.size, g.spans.data_ptr()) == data.size
        a, body, z, sp = g.host()
        assert (a == sm.POISON).all() and (z == sm.POISON).all()
        assert sp[:, 1].tolist() == [int(x) for x in want], algo
        assert (body == data).all()
        m = fs.close_file(h)
        assert m["chunk_time"] > 0 and m["hash_time"] > 0
    assert sorted(fs.list_files()) == ["random", "zeros"]
    if algo == "fast":  # a CUDA tensor written with no host copy equals the same bytes from the host
        data = oracle.splitmix64_bytes(MB, 1234)
        t = torch.from_numpy(data).cuda()
        h = fs.create_file("tensor", ch)
        fs.write_to_file(h, t)
        r = fs.open_file_readonly("random")
        assert (fs.hashes(h) == fs.hashes(r)).all()
        assert (fs.read_file_complete(h) == data).all()
        assert fs.stat(h)["size"] == fs.stat(r)["size"] == MB


# ---- refusals ---------------------------------------------------------------------------------
def test_short_buffers_write_nothing():
    import chunkfs_amd as c
    rng = np.random.default_rng(37)
    data = rng.integers(0, 256, 10000, dtype=np.uint8)
    p = Pair(c, seg=4096)
    w = p.create("f")
    p.append(w, data, _tiling([1000] * 10))
    r = p.open("f", readonly=True)
    g = sm.Guarded(10000, 10)
    assert p.fs.read_complete_device(r[0], g.out_ptr, 9999, g.spans.data_ptr()) == 10000
    assert p.fs.read_complete_device(r[0], None, 0) == 10000  # sizes a read
    assert p.fs.read_device(r[0], g.out_ptr, 3999) == 4000
    assert p.fs.read_device(r[0], None, 0) == 4000
    g.assert_untouched()
    assert p.fs.stat(r[0])["cursor"] == 0  # a refused segment read leaves the cursor
    assert p.read_segment(r).size == 4000
    L = c._lib.lib()
    assert L.cdc_file_hashes_device(r[0]._fh, ctypes.c_void_p(g.out_ptr), 9) == 10
    g.assert_untouched()


def test_refused_write_changes_nothing():
    import chunkfs_amd as c
    ch = c.FSChunker(4096)
    fs = c.FileSystem(max_chunks=256, arena_bytes=100 * 4096)
    rng = np.random.default_rng(41)
    first, second = (rng.integers(0, 256, 60 * 4096, dtype=np.uint8) for _ in range(2))
    h = fs.create_file("f", ch)
    assert fs.write_to_file(h, first) == 60
    before, store_before = fs.stat(h), fs.store.stats()
    with pytest.raises(c.CdcError) as ei:
        fs.write_to_file(h, second)  # 60 more chunks do not fit the arena
    assert _code(ei) == c._lib.CDC_ENOMEM
    after = fs.stat(h)
    assert (after["size"], after["spans"]) == (before["size"], before["spans"]) and fs.store.stats() == store_before
    d_data, dc, dd = sm.dev(second), sm.dev_chunks([[second.size - 10, 11]]), sm.dev(np.zeros((1, 32), np.uint8))
    with pytest.raises(c.CdcError) as ei:  # a chunk that leaves its buffer
        fs.append_device(h, d_data.data_ptr(), second.size, dc.data_ptr(), dd.data_ptr(), 1)
    assert _code(ei) == c._lib.CDC_EINVAL
    assert fs.stat(h)["spans"] == 60 and fs.store.stats() == store_before
    assert fs.write_to_file(h, second[:40 * 4096]) == 40  # one that fits is taken
    assert (fs.read_file_complete(h) == np.concatenate([first, second[:40 * 4096]])).all()


def test_store_cleared_under_the_layer():
    import chunkfs_amd as c
    rng = np.random.default_rng(43)
    data = rng.integers(0, 256, 5000, dtype=np.uint8)
    p = Pair(c, seg=4096)
    w = p.create("f")
    p.append(w, data, _tiling([1000] * 5))
    r = p.open("f", readonly=True)
    p.fs.store.clear()  # directly, not through the layer
    g = sm.Guarded(5000, 5)
    calls = [lambda: p.fs.read_complete_device(r[0], g.out_ptr, 5000, g.spans.data_ptr()),
             lambda: p.fs.read_device(r[0], g.out_ptr, 5000),
             lambda: p.fs.pread_device(r[0], 10, 100, g.out_ptr),
             lambda: p.fs.pread_batch_device([(r[0], 10, 100, g.out_ptr)]),
             lambda: p.fs.chunk_count_distribution(r[0]),
             lambda: p.append(w, data, [[0, 10]])]
    for call in calls:
        with pytest.raises(c.CdcError) as ei:
            call()
        assert _code(ei) == c._lib.CDC_ENOTFOUND
    g.assert_untouched()
    assert p.fs.stat(r[0])["size"] == 5000 and p.fs.store.stats()["chunks_written"] == 0
    fresh = p.fs.create_file("f", None)  # a file written after the clear reads fine
    d_data, dc, dd = sm.dev(data), sm.dev_chunks([[5, 50]]), sm.dev(_digests(data, [[5, 50]]))
    p.fs.append_device(fresh, d_data.data_ptr(), data.size, dc.data_ptr(), dd.data_ptr(), 1)
    assert (p.fs.read_file_complete(r[0]) == data[5:55]).all()


def test_clear_database():
    import chunkfs_amd as c
    rng = np.random.default_rng(47)
    data = rng.integers(0, 256, 5000, dtype=np.uint8)
    p = Pair(c)
    w, w2 = p.create("f"), p.create("g")
    p.append(w, data, _tiling([2500, 2500]))
    r = p.open("f", readonly=True)
    p.fs.clear_database()
    p.m.clear()
    assert p.fs.list_files() == [] and not p.fs.file_exists("f")
    s = p.fs.store.stats()
    assert s["chunks_written"] == 0 and s["arena_used"] == 0
    g = sm.Guarded(5000, 2)
    for call in (lambda: p.fs.stat(r[0]), lambda: p.fs.read_complete_device(r[0], g.out_ptr, 5000),
                 lambda: p.fs.read_device(w[0], g.out_ptr, 5000), lambda: p.fs.pread_device(r[0], 0, 10, g.out_ptr),
                 lambda: p.append(w2, data, [[0, 10]]), lambda: p.fs.hashes(r[0]), lambda: p.fs.close_file(w[0])):
        with pytest.raises(c.CdcError) as ei:
            call()
        assert _code(ei) == c._lib.CDC_ENOTFOUND
    g.assert_untouched()
    again = p.create("f")
    p.append(again, data, [[100, 200]])
    p.check_file(again)


# ---- stream order --------------------------------------------------------------------------------
def test_stream_order_on_a_user_stream():
    """Work queued on a user stream ahead of a write and ahead of a read, no host wait in between."""
    import torch
    import chunkfs_amd as c
    n = MB
    data = oracle.splitmix64_bytes(n, 4243)
    src = sm.dev(data)
    fs = c.FileSystem(max_chunks=1 << 10, arena_bytes=2 * MB)
    h = fs.create_file("f", c.FastChunker(c.SizeParams(4096, 8192, 16384)))
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    back = torch.zeros(n + 2, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(20):  # keep the stream busy ahead of the copy the write depends on
            buf.add_(1)
        buf.copy_(src)
    spans = fs.write_to_file(h, buf, stream=s.cuda_stream)
    with torch.cuda.stream(s):
        back.fill_(0x5A)  # queued ahead of the read: must not land on top of it
    assert fs.read_complete_device(h, back.data_ptr() + 1, n, stream=s.cuda_stream) == n
    assert spans == len(oracle.fastcdc(data, 4096, 8192, 16384))
    got = back.cpu().numpy()
    assert got[0] == 0x5A and got[-1] == 0x5A and (got[1:-1] == data).all()


# ---- scratch that grows between calls ------------------------------------------------------------------
def _pread_batch(p, hm, nreq, rng):
    """One pread_batch of nreq ranges of the file into one guarded buffer, against the model."""
    import torch
    size = p.m.size(hm[1])
    reqs = [(0, size)] + [(int(rng.integers(0, size)), int(rng.integers(1, 2000))) for _ in range(nreq - 1)]
    at, places = sm.GUARD, []
    for i, (_, ln) in enumerate(reqs):
        at += (i * 7) % 16  # every alignment
        places.append(at)
        at += ln + 32
    image = np.full(at + sm.GUARD, sm.POISON, dtype=np.uint8)
    buf = torch.full((image.size,), sm.POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    want = []
    for (off, ln), where in zip(reqs, places):
        w = p.m.pread(hm[1], off, ln)
        image[where:where + w.size] = w
        want.append(w.size)
    got = p.fs.pread_batch_device([(hm[0], off, ln, buf.data_ptr() + where) for (off, ln), where in zip(reqs, places)])
    assert got == want
    assert (buf.cpu().numpy() == image).all()


def _verify(p, hm, data):
    import torch
    d = sm.dev(data)
    assert p.fs.verify_device(hm[0], d.data_ptr(), data.size) == (True, None)
    d[data.size // 3] ^= 1
    torch.cuda.synchronize()
    assert p.fs.verify_device(hm[0], d.data_ptr(), data.size) == (False, data.size // 3)


def test_every_call_small_then_large_then_small_again():
    """The layer keeps its scratch between calls and frees and reallocates a
    group when a call needs more.  Every kind of call at a size the first
    allocation holds (a file of about 3 spans, one request), then at sizes that
    outgrow every group (200 spans and more against the n + n/8 + 64 of a
    3-span call, 48 requests and 20 files in a batch against the n + n/8 + 16
    of one, a splice window past the first 4096-byte buffer), then small again:
    all of it against the models.  A second layer does the same for the reads
    that go through target-kind containers, which the edits refuse."""
    import chunkfs_amd as c
    import bench_model as bm
    import splice_model as spm
    from test_gpu_snapshot import Driver  # imports this module, so not at its top
    from test_gpu_splice import SPair

    def layer():
        return c.FileSystem.new_with_scrubber(c.CopyScrubber(), max_chunks=1 << 12, arena_bytes=4 * MB,
                                              target_max_chunks=1 << 12, target_arena_bytes=4 * MB, seg_size=8192)

    d = Driver(c, "fast", fs=layer())  # the target is attached, nothing is scrubbed: every call is allowed
    p = d.p
    rng = np.random.default_rng(61)

    def every_call(tag, size, nreq, nfiles, ins_len, seed):
        data = spm.rand(seed, size)
        a = d.file(tag + "_a", data)  # write
        spans = p.fs.stat(a[0])["spans"]
        names = [f"{tag}_b{i}" for i in range(nfiles)]  # batch write
        hms = [p.create(name, p.chunker) for name in names]
        datas = [spm.rand(seed + 1 + i, 300 + 40 * i) for i in range(nfiles)]
        chunks = [spm.chunk("fast", x) for x in datas]
        assert p.fs.write_to_files([h for h, _ in hms], datas) == [len(ch) for ch in chunks]
        for name, hm, x, ch in zip(names, hms, datas, chunks):
            p.m.append(hm[1], x, ch)
            p.seen.update(p.m.hashes(hm[1]))
            p.open_files[name] = hm
        _pread_batch(p, a, nreq, rng)
        assert (p.check_file(a, shift=3) == data).all()  # read_complete with its spans
        r = p.open(tag + "_a", readonly=True)
        p.read_segment(r)
        _verify(p, a, data)
        assert p.fs.chunk_count_distribution(a[0]) == p.m.distribution(a[1])
        derived = p.fs.get_to_dedup_ratio(tag + "_a", 2.0)
        assert derived == bm.get_to_dedup_ratio(p.m, tag + "_a", 2.0)
        p.check_file(p.open(derived, readonly=True))
        b = d.clone(tag + "_a", tag + "_c")
        d.splice(b, size // 2, 5, spm.rand(seed + 50, ins_len))  # a new table, and the file against the model
        d.splice(b, size // 4, 3, spm.rand(seed + 51, 3))
        assert d.diff(a, b)["n_ranges"] >= 1
        d.diff(a, b, tables_only=True)
        p.remove(names[0])
        p.collect()
        for hm in [a, b] + hms[1:]:
            p.check_file(hm)
        return spans

    assert 2 <= every_call("small", 700, 1, 1, 10, 100) <= 6
    assert every_call("large", 96 << 10, 48, 20, 3000, 200) >= 200
    assert 2 <= every_call("again", 700, 1, 1, 10, 300) <= 6
    p.check_store()

    # The reads through target-kind containers: small, scrub, read; large, scrub, read; small again.
    q = SPair(c, "fast", fs=layer())
    small, large = spm.rand(400, 700), spm.rand(401, 96 << 10)
    s1 = q.new_file("s1", small)
    assert q.fs.scrub().processed_data > 0

    def scrubbed_reads(hm, data, nreq):
        _pread_batch(q, hm, nreq, rng)
        assert (q.check_file(hm, shift=5) == data).all()
        _verify(q, hm, data)

    scrubbed_reads(s1, small, 1)
    s2 = q.new_file("s2", large)
    assert q.fs.stat(s2[0])["spans"] >= 200 and q.fs.scrub().processed_data > 0
    assert q.fs.store.scrub_stats()["chunk_containers"] == 0
    scrubbed_reads(s2, large, 48)
    scrubbed_reads(s1, small, 1)


# ---- the C++ mirror ---------------------------------------------------------------------------------
def test_cpp_files_mirror_runs():
    from chunkfs_amd import _lib, build
    exe = os.path.join(ROOT, "_build", "files_example")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "examples", "store_example.cpp"),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd", "-L", os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
                    "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "files ok: 2 files, pread 5000 bytes at 60000" in r.stdout
