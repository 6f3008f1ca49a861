"""Scrub stage (include/chunkfs_amd.h "Scrub stage") on the GPU, through the
Python mirror, bit for bit against tests/scrub_model.py: CopyScrubber /
DumbScrubber as the reference has them (src/system/scrub.rs:85-129), this
project's RechunkScrubber, retrieve through target keys
(src/system/storage.rs:141-157), the statistics (storage.rs:193-261) and the
clears (src/system/mod.rs:271-298).  Every output buffer is guarded by poisoned
bytes (store_model.Guarded)."""
import hashlib
import math
import os

import numpy as np
import pytest

import oracle
import scrub_model as scm
import store_model as sm
from test_gpu_files import Pair

pytestmark = pytest.mark.gpu
MB = 1 << 20
EINVAL, ENOMEM, ENOTFOUND = -1, -2, -5
FAST, RABIN = (64, 256, 1024), (64, 256, 1024)  # rabin: a size set of tests/test_gpu_walk.py
SCRUBBERS = ["copy", "dumb", "fixed512", "fast", "rabin"]


def _sub_chunks(kind):
    """The oracle's chunk_data of a container's bytes for a RECHUNK scrubber."""
    def run(b):
        a = np.frombuffer(b, dtype=np.uint8)
        if a.size == 0:
            return []
        if kind == "fixed512":
            return oracle.fixed(a.size, 512)
        return oracle.fastcdc(a, *FAST) if kind == "fast" else oracle.cdc("rabin", a, *RABIN)
    return run


def _scrubber(c, kind):
    if kind == "copy":
        return c.CopyScrubber()
    if kind == "dumb":
        return c.DumbScrubber()
    if kind == "fixed512":
        return c.RechunkScrubber(c.FSChunker(512))
    if kind == "fast":
        return c.RechunkScrubber(c.FastChunker(c.SizeParams(*FAST)))
    return c.RechunkScrubber(c.RabinChunker(c.SizeParams(*RABIN)))


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


class ScrubPair(Pair):
    """A file system with a scrubber and the model, driven side by side."""

    def __init__(self, c, kind, seg=4096, max_chunks=1 << 12, arena=4 * MB, t_max_chunks=1 << 14, t_arena=4 * MB):
        self.c, self.kind, self.seg = c, kind, seg
        self.fs = c.FileSystem.new_with_scrubber(_scrubber(c, kind), max_chunks=max_chunks, arena_bytes=arena,
                                                 target_max_chunks=t_max_chunks, target_arena_bytes=t_arena,
                                                 seg_size=seg)
        self.m = scm.FileSystem(seg_size=seg)

    def scrub(self):
        got = self.fs.scrub()
        ms = self.m.store
        want = (ms.scrub_copy() if self.kind == "copy" else ms.scrub_dumb() if self.kind == "dumb"
                else ms.scrub_rechunk(_sub_chunks(self.kind)))
        assert (got.processed_data, got.data_left) == (want.processed_data, want.data_left)
        assert got.running_time > 0 or self.kind == "dumb"
        return got

    def check_store(self, seed=0):
        """get_device, storage_iterator, scrub_stats, the ratios and the counters, against the model."""
        ms, store = self.m.store, self.fs.store
        digests = list(ms.base)
        rng = np.random.default_rng(seed)
        if digests:
            order = rng.integers(0, len(digests), size=len(digests) + 7)  # shuffled, with repeats
            req = np.array([np.frombuffer(digests[i], dtype=np.uint8) for i in order])
            for shift in (0, 1, 13):
                sm.get_checked(store, ms, req, shift)
            assert store.contains_device(sm.dev(req).data_ptr(), len(req)) == len(req)
        it = {d: (kind, ln, keys) for d, kind, ln, keys in self.fs.storage_iterator()}
        assert it == ms.iterator()
        assert self.fs.store.scrub_stats() == ms.scrub_stats()
        st = store.stats()
        for k, v in ms.stats().items():
            assert st[k] == v, (k, st[k], v)
        assert _same(self.fs.cdc_dedup_ratio(), ms.cdc_dedup_ratio())
        assert _same(self.fs.full_cdc_dedup_ratio(), ms.full_cdc_dedup_ratio())
        assert _same(self.fs.total_dedup_ratio(), ms.total_dedup_ratio())
        if ms.base:
            assert self.fs.average_chunk_size() == ms.average_chunk_size()
        return it

    def check_reads(self, name):
        """read_file_complete with spans and hashes, then read_from_file looped to the end."""
        want = self.check_file(self.open(name, readonly=True), shift=3)
        r = self.open(name, readonly=True)
        parts = []
        while True:
            part = self.read_segment(r)
            if part.size == 0:
                break
            parts.append(part)
        if parts:
            got = np.concatenate(parts)
            assert (got == want[:got.size]).all()
        return want

    def snapshot(self, names):
        """Everything a refused call must leave alone (the counters: a ratio may be nan)."""
        def ints(d):
            return {k: v for k, v in d.items() if isinstance(v, int)}
        return (ints(self.fs.store.stats()), ints(self.fs.target.stats()), self.fs.store.scrub_stats(),
                sorted(self.fs.storage_iterator()), [self.fs.read_file_complete(self.fs.open_file_readonly(n)).tobytes()
                                                     for n in names])


def _dup_data(n=256 << 10):
    a = oracle.splitmix64_bytes(n // 2, 7)
    return np.concatenate([a, a[n // 8:n // 4], oracle.splitmix64_bytes(n // 2 - n // 8, 8)])


def _base(c, base):
    if base == "fixed4096":
        return c.FSChunker(4096), lambda d: oracle.fixed(d.size, 4096)[:, 1]
    return c.FastChunker(c.SizeParams(*FAST)), lambda d: oracle.fastcdc(d, *FAST)[:, 1]


# ---- 1. all scrubbers against all reads -----------------------------------------------
@pytest.mark.parametrize("kind", SCRUBBERS)
@pytest.mark.parametrize("base", ["fixed4096", "fast"])
def test_every_scrubber_against_every_read(base, kind):
    import chunkfs_amd as c
    data = _dup_data()
    assert data.size == 256 << 10
    ch, lengths = _base(c, base)
    p = ScrubPair(c, kind)
    w = p.create("f", ch)
    p.write(w, data, lengths(data))
    p.check_store()
    before = p.fs.cdc_dedup_ratio()
    assert before > 1
    p.scrub()
    it = p.check_store(1)
    assert (p.check_reads("f") == data).all()
    ss = p.fs.store.scrub_stats()
    st = p.fs.store.stats()
    if kind == "dumb":
        assert ss["target_containers"] == 0 and st["arena_used"] > 0
        return
    assert ss["chunk_containers"] == 0 and st["arena_used"] == 0 and p.fs.cdc_dedup_ratio() == math.inf
    if kind == "copy":
        assert p.fs.total_dedup_ratio() == before
        return
    # RECHUNK: every key list is the oracle's chunking of the container's bytes plus hashlib
    sub = _sub_chunks(kind)
    for d, (k, ln, keys) in it.items():
        b = p.m.store.retrieve([d])[0]
        assert k == "target" and ln == len(b) and hashlib.sha256(b).digest() == d
        assert keys == [hashlib.sha256(b[int(o):int(o) + int(n)]).digest() for o, n in sub(b)]


# ---- 2. pread edges after RECHUNK ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["fixed512", "fast"])
def test_pread_edges_after_rechunk(kind):
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(5 * 4096 + 1234, 21)
    p = ScrubPair(c, kind)
    w = p.create("f", c.FSChunker(4096))
    p.write(w, data, oracle.fixed(data.size, 4096)[:, 1])
    p.scrub()
    r = p.open("f", readonly=True)
    size = data.size
    subs = [4096 + int(o) for o, _ in _sub_chunks(kind)(data[4096:8192].tobytes())]  # sub-chunk starts in container 1
    s1, s2 = subs[1], subs[2]
    ranges = [(s1 + 3, 5), (s1 - 7, 30),            # inside a sub-chunk; across a sub-chunk boundary
              (s1, s2 - s1), (s1, 1), (s1 - 1, 1),  # exactly a sub-chunk; its first byte; the byte before
              (s1 + 1, s2 - s1 - 1), (s1 - 5, 5),   # ends exactly on a sub-chunk boundary
              (4096, 4096), (8192, 100), (100, 3996),  # exactly a container; starts on / ends on its boundary
              (4090, 12), (4000, 4300), (1, 3 * 4096),  # across two containers and more
              (0, size), (size - 1, 1), (size - 5, 100), (size, 10), (size + 9, 1), (7, 0), (0, 1)]
    for i, (off, ln) in enumerate(ranges):
        want = p.pread(r, off, ln, shift=i % 3)
        assert (want == data[off:off + ln]).all()
    # pread_batch over two files: one written before the scrub, one after it (chunk-kind)
    late = oracle.splitmix64_bytes(3 * 4096 + 77, 22)
    w2 = p.create("late", c.FSChunker(4096))
    p.write(w2, late, oracle.fixed(late.size, 4096)[:, 1])
    r2 = p.open("late", readonly=True)
    reqs = [(r, s1 - 9, 700), (r2, 4090, 4200), (r, size - 3, 50), (r2, 0, late.size), (r, 0, 0), (r2, 5000, 1)]
    bufs = [sm.Guarded(ln, 0, i % 2) for i, (_, _, ln) in enumerate(reqs)]
    got = p.fs.pread_batch_device([(h[0], off, ln, g.out_ptr) for (h, off, ln), g in zip(reqs, bufs)])
    for (h, off, ln), g, n in zip(reqs, bufs, got):
        want = p.m.pread(h[1], off, ln)
        a, body, z, _ = g.host()
        assert n == want.size and (body[:n] == want).all() and (body[n:] == sm.POISON).all()
        assert (a == sm.POISON).all() and (z == sm.POISON).all()
    p.check_store()


# ---- 3. container shapes ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["copy", "fixed512", "fast"])
def test_container_shapes(kind):
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(8192, 31)
    chunks = [[0, 0], [0, 100], [100, 1000], [1100, 777], [0, 100], [2000, 513], [100, 1000], [3000, 1],
              [0, 0], [4000, 512], [0, 100]]  # length 0; shorter than a sub-chunk; no multiples of 16; repeats
    p = ScrubPair(c, kind)
    w = p.create("f", None)
    p.append(w, data, chunks)
    p.scrub()
    it = p.check_store()
    if kind != "copy":
        assert it[hashlib.sha256(b"").digest()] == ("target", 0, [])  # a length-0 chunk: zero keys
    if kind == "fixed512":
        assert len(it[hashlib.sha256(data[:100].tobytes()).digest()][2]) == 1
    p.check_reads("f")
    r = p.open("f", readonly=True)
    for off, ln in ((0, 100), (99, 2), (100, 1000), (611, 2), (1877, 200), (0, 10000)):
        p.pread(r, off, ln)


def test_one_three_mib_chunk_becomes_6144_keys():
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(3 * MB, 41)
    p = ScrubPair(c, "fixed512", seg=4 * MB, arena=4 * MB, t_arena=4 * MB)
    w = p.create("big", None)
    p.append(w, data, [[0, data.size]])
    p.scrub()
    it = p.check_store()
    assert [len(k) for _, _, k in it.values()] == [6144]
    assert (p.check_reads("big") == data).all()
    r = p.open("big", readonly=True)
    for off, ln in ((511, 2), (MB - 1, 513), (3 * MB - 700, 9999), (123457, 2 * MB)):
        p.pread(r, off, ln, shift=1)


@pytest.mark.parametrize("kind", ["copy", "fixed512"])
def test_many_writes_of_few_chunks(kind):
    """Thousands of writes of three chunks into a small table: the scrub lists three containers."""
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(4096, 43)
    p = ScrubPair(c, kind, seg=MB, max_chunks=64)  # 1024 slots
    w = p.create("f", None)
    for _ in range(150):  # a put takes at most max_chunks chunks, "as if every chunk were new"
        p.append(w, data, [[0, 700], [700, 1300], [0, 700]] * 20)
    p.append(w, data, [[2000, 2096]])
    assert p.fs.store.stats()["chunks_written"] == 9001 > 8 * 1024
    p.scrub()
    it = p.check_store()
    assert len(it) == 3
    assert p.check_reads("f").size == 3000 * 2700 + 2096


# ---- 4. groups ------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["3", "1000,9000"])  # 3 containers a group; the byte bound cuts groups
def test_groups_give_the_same_result(group):
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(10 * 4096 - 100, 51)
    results = []
    for env in (None, group):
        old = os.environ.pop("CHUNKFS_AMD_SCRUB_GROUP", None)
        if env is not None:
            os.environ["CHUNKFS_AMD_SCRUB_GROUP"] = env
        try:
            p = ScrubPair(c, "fast")
            w = p.create("f", c.FSChunker(4096))
            p.write(w, data, oracle.fixed(data.size, 4096)[:, 1])
            assert p.fs.store.stats()["unique_chunks"] == 10
            p.scrub()
        finally:
            os.environ.pop("CHUNKFS_AMD_SCRUB_GROUP", None)
            if old is not None:
                os.environ["CHUNKFS_AMD_SCRUB_GROUP"] = old
        it = p.check_store()
        assert (p.check_reads("f") == data).all()
        results.append((it, p.fs.store.scrub_stats(), p.fs.target.stats()["unique_bytes"]))
    assert results[0] == results[1]


# ---- 5. sequences -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["copy", "fixed512"])
def test_write_scrub_write_read_and_a_second_scrub(kind):
    import chunkfs_amd as c
    a = oracle.splitmix64_bytes(6 * 4096, 61)
    ch = c.FSChunker(4096)
    p = ScrubPair(c, kind)
    w = p.create("a", ch)
    p.write(w, a, oracle.fixed(a.size, 4096)[:, 1])
    r = p.open("a", readonly=True)
    first = p.read_segment(r)  # one span: the cursor is mid-file when the scrub runs
    assert first.size == 4096
    assert p.scrub().processed_data == a.size
    # duplicates of scrubbed chunks plus new data
    b = np.concatenate([a[4096:3 * 4096], oracle.splitmix64_bytes(2 * 4096 + 5, 62)])
    w2 = p.create("b", ch)
    p.write(w2, b, oracle.fixed(b.size, 4096)[:, 1])
    ss = p.fs.store.scrub_stats()
    assert ss["chunk_containers"] == 3 and ss["cdc_bytes"] == 2 * 4096 + 5
    assert p.fs.store.stats()["arena_used"] == 2 * 4096 + 16  # the arena fills again from the start
    p.check_store()
    assert (p.check_reads("a") == a).all() and (p.check_reads("b") == b).all()
    rest = [first]
    while True:  # the handle opened before the scrub goes on from its cursor
        part = p.read_segment(r)
        if part.size == 0:
            break
        rest.append(part)
    assert (np.concatenate(rest) == a).all()
    assert p.scrub().processed_data == 2 * 4096 + 5  # only the new chunk bytes
    assert p.fs.scrub().processed_data == 0 and p.fs.store.scrub_stats()["chunk_containers"] == 0
    p.check_store()
    assert (p.check_reads("a") == a).all() and (p.check_reads("b") == b).all()


@pytest.mark.parametrize("kind", ["copy", "fast"])
def test_clears(kind):
    import chunkfs_amd as c
    data = _dup_data(64 << 10)
    ch = c.FSChunker(4096)
    lengths = oracle.fixed(data.size, 4096)[:, 1]
    p = ScrubPair(c, kind)
    w = p.create("f", ch)
    p.write(w, data, lengths)
    p.scrub()
    target = p.fs.target.stats()
    # clear_database keeps the target; rewrite + scrub adds no target value
    p.fs.clear_database()
    p.m.clear()
    assert p.fs.target.stats() == target and p.fs.list_files() == []
    p.check_store()
    with pytest.raises(c.CdcError) as ei:
        p.fs.read_file_complete(w[0])
    assert ei.value.code == ENOTFOUND
    w = p.create("f", ch)
    p.write(w, data, lengths)
    p.check_store()
    p.scrub()
    assert p.fs.target.stats()["unique_chunks"] == target["unique_chunks"]
    assert p.fs.target.stats()["unique_bytes"] == target["unique_bytes"]
    p.check_store()
    assert (p.check_reads("f") == data).all()
    # clear_file_system empties both
    p.fs.clear_file_system()
    p.m.clear_file_system()
    assert p.fs.target.stats()["unique_chunks"] == 0 and p.fs.store.stats()["unique_chunks"] == 0
    p.check_store()
    w = p.create("f", ch)
    p.write(w, data, lengths)
    p.scrub()
    p.check_store()
    assert (p.check_reads("f") == data).all()


@pytest.mark.parametrize("kind", ["copy", "fixed512", "fast"])
def test_scrub_of_an_empty_store(kind):
    """A fresh file system, and one just after clear_file_system and after clear_database: no
    container to list.  All-zero measurements, nothing changes, and the pair works afterwards."""
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(3 * 4096 + 9, 65)
    ch = c.FSChunker(4096)
    p = ScrubPair(c, kind)
    assert p.scrub().processed_data == 0  # nothing was ever written
    p.check_store()
    assert p.fs.storage_iterator() == [] and p.fs.store.scrub_stats()["keys"] == 0
    for clear in ("clear_file_system", "clear_database"):
        w = p.create("f", ch)
        p.write(w, data, oracle.fixed(data.size, 4096)[:, 1])
        assert p.scrub().processed_data == data.size
        assert (p.check_reads("f") == data).all()
        if clear == "clear_file_system":
            p.fs.clear_file_system()
            p.m.clear_file_system()
        else:
            p.fs.clear_database()
            p.m.clear()
        assert p.scrub().processed_data == 0
        assert p.fs.scrub().processed_data == 0
        p.check_store()
        assert p.fs.storage_iterator() == []


def test_clearing_the_target_directly():
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(4 * 4096, 71)
    ch = c.FSChunker(4096)
    p = ScrubPair(c, "fixed512")
    w = p.create("f", ch)
    p.write(w, data, oracle.fixed(data.size, 4096)[:, 1])
    p.scrub()
    late = oracle.splitmix64_bytes(4096, 72)
    w2 = p.create("late", ch)
    p.write(w2, late, [4096])  # chunk-kind: needs no target
    p.fs.target.clear()
    digs = sm.dev(np.array([np.frombuffer(d, dtype=np.uint8) for d in p.m.store.base]))
    g = sm.Guarded(data.size + late.size, 5)
    with pytest.raises(c.CdcError) as ei:
        p.fs.store.get_device(digs.data_ptr(), 5, g.out_ptr, g.nbytes, g.spans.data_ptr())
    assert ei.value.code == ENOTFOUND
    g.assert_untouched()
    g = sm.Guarded(data.size, 4)
    for call in (lambda: p.fs.read_complete_device(w[0], g.out_ptr, g.nbytes, g.spans.data_ptr()),
                 lambda: p.fs.pread_device(w[0], 10, 100, g.out_ptr),
                 lambda: p.fs.read_device(p.fs.open_file_readonly("f"), g.out_ptr, g.nbytes),
                 lambda: p.fs.scrub(), lambda: p.fs.storage_iterator()):
        with pytest.raises(c.CdcError) as ei:
            call()
        assert ei.value.code == ENOTFOUND
    g.assert_untouched()
    assert (p.fs.read_file_complete(w2[0]) == late).all()  # chunk-kind data is still there
    g1 = sm.Guarded(4096, 1)
    assert p.fs.read_complete_device(w2[0], g1.out_ptr, 4096, g1.spans.data_ptr()) == 4096
    assert g1.host()[3].tolist() == [[0, 4096]]
    # a later clear_database makes the pair usable again
    p.fs.clear_database()
    p.m.clear_file_system()  # the target was emptied by hand
    w = p.create("f", ch)
    p.write(w, data, oracle.fixed(data.size, 4096)[:, 1])
    p.scrub()
    p.check_store()
    assert (p.check_reads("f") == data).all()


# ---- 6. refusal -----------------------------------------------------------------------------------
def _need(p, kind):
    """Keys and padded bytes a scrub asks of the target, as if every key were new."""
    sub = _sub_chunks(kind) if kind != "copy" else (lambda b: [(0, len(b))])
    lens = [int(n) for kd, v in p.m.store.base.values() if kd == scm.CHUNK for _, n in sub(v)]
    return len(lens), sum(sm.round_up16(n) for n in lens)


@pytest.mark.parametrize("group", [None, "3"])
@pytest.mark.parametrize("short", ["max_chunks", "arena"])
@pytest.mark.parametrize("kind", ["copy", "fixed512"])
def test_a_refused_scrub_changes_nothing(kind, short, group):
    import chunkfs_amd as c
    # Containers of the same eight 512-byte blocks in other orders: few distinct keys, counted "as if every key were new".
    pool = oracle.splitmix64_bytes(4096, 81).reshape(8, 512)
    data = np.concatenate([pool[np.roll(np.arange(8), i)].reshape(-1) for i in range(7)] +
                          [oracle.splitmix64_bytes(300, 82)])
    lengths = oracle.fixed(data.size, 4096)[:, 1]
    probe = ScrubPair(c, kind)
    probe.write(probe.create("f", c.FSChunker(4096)), data, lengths)
    keys, padded = _need(probe, kind)
    old = os.environ.pop("CHUNKFS_AMD_SCRUB_GROUP", None)
    if group is not None:
        os.environ["CHUNKFS_AMD_SCRUB_GROUP"] = group
    try:
        for fits in (False, True):
            p = ScrubPair(c, kind, t_max_chunks=keys - (short == "max_chunks" and not fits),
                          t_arena=padded - 16 * (short == "arena" and not fits))
            p.write(p.create("f", c.FSChunker(4096)), data, lengths)
            before = p.snapshot(["f"])
            if fits:
                p.scrub()
                p.check_store()
                assert (p.check_reads("f") == data).all()
                continue
            with pytest.raises(c.CdcError) as ei:
                p.fs.scrub()
            assert ei.value.code == ENOMEM
            assert p.snapshot(["f"]) == before
            p.check_store()
            assert (p.check_reads("f") == data).all()
    finally:
        os.environ.pop("CHUNKFS_AMD_SCRUB_GROUP", None)
        if old is not None:
            os.environ["CHUNKFS_AMD_SCRUB_GROUP"] = old


def test_set_target_rules():
    import chunkfs_amd as c
    p = ScrubPair(c, "copy")
    data = oracle.splitmix64_bytes(8192, 91)
    p.write(p.create("f", c.FSChunker(4096)), data, [4096, 4096])
    other = c.ChunkStore(64, 1 << 16)
    p.fs.store.set_target(other)  # no target-kind containers yet: allowed
    p.fs.store.set_target(p.fs.target)
    p.scrub()
    for bad in (other, p.fs.target):
        with pytest.raises(c.CdcError) as ei:
            p.fs.store.set_target(bad)  # target-kind containers exist
        assert ei.value.code == EINVAL
    with pytest.raises(c.CdcError) as ei:
        other.set_target(p.fs.store)  # the target has a target itself
    assert ei.value.code == EINVAL
    with pytest.raises(c.CdcError) as ei:
        other.set_target(other)
    assert ei.value.code == EINVAL
    p.check_store()


# ---- 7. no target attached ----------------------------------------------------------------------------
def test_no_target_attached():
    import chunkfs_amd as c
    store = c.ChunkStore(64, 1 << 16)
    for s in (c.CopyScrubber(), c.DumbScrubber(), c.RechunkScrubber(c.FSChunker(512))):
        with pytest.raises(c.CdcError) as ei:
            store.scrub(s)
        assert ei.value.code == EINVAL
    fs = c.FileSystem(max_chunks=64, arena_bytes=1 << 16, seg_size=4096)
    data = oracle.splitmix64_bytes(10000, 92)
    h = fs.create_file("f", c.FSChunker(4096))
    assert fs.write_to_file(h, data) == 3
    assert (fs.read_file_complete(h) == data).all()
    assert (fs.pread(h, 4000, 200) == data[4000:4200]).all()
    with pytest.raises(c.CdcError) as ei:
        fs.scrub()
    assert ei.value.code == EINVAL
    st = fs.store.stats()
    assert st["cdc_dedup_ratio"] == 1.0 and fs.store.scrub_stats()["cdc_bytes"] == st["unique_bytes"] == 10000
    assert sorted((k, ln, keys) for _, k, ln, keys in fs.storage_iterator()) == [("chunk", 1808, [])] + [("chunk", 4096, [])] * 2
