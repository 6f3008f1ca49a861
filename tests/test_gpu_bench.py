"""Bench fixture (include/chunkfs_amd.h "Bench fixture") on the GPU, through the
Python mirror, against tests/bench_model.py: derived files with a chosen dedup
ratio (src/system/file_layer.rs:208-268), verification of a file against a
dataset in HBM and the store's size histogram (src/bench/mod.rs:218-275), and
chunkfs_amd.bench.CDCFixture on top of them.  Device and model are driven side
by side (test_gpu_files.Pair); device outputs are guarded by poison."""
import ctypes
import math

import numpy as np
import pytest

import bench_model as bm
import files_model as fm
import oracle
import scrub_model as scm
import store_model as sm
from test_gpu_files import Pair
from test_gpu_scrub import ScrubPair

pytestmark = pytest.mark.gpu
MB = 1 << 20
EINVAL, ENOTFOUND = -1, -5
FAST = (4096, 8192, 16384)

DATA = oracle.splitmix64_bytes(460, 77)
# 12 spans, lengths 0..100, duplicates of (0, 40), (40, 60) and of the empty chunk; the first unique entry is
# empty, so it sits at every cycle wrap.  Unique over spans 0..10: [0, 40, 60, 100, 1, 99, 77, 23], 400 bytes.
SPEC_WRAP = [(0, 0), (0, 40), (40, 60), (0, 40), (100, 100), (200, 1), (201, 99), (40, 60), (300, 0), (300, 77),
             (377, 23), (400, 50)]
# The same without the leading empty span.  Unique: [40, 60, 100, 1, 99, 0, 77, 23, 50], 450 bytes.
SPEC_PLAIN = SPEC_WRAP[1:] + [(450, 10)]
SPECS = {"none": [], "one": [(0, 10)], "two": [(0, 10), (10, 25)], "wrap": SPEC_WRAP, "plain": SPEC_PLAIN}


def _code(excinfo):
    return excinfo.value.code


def _build(p, name, chunks, data=DATA):
    w = p.create(name)
    if len(chunks):
        p.append(w, data, chunks)
    return w


def _derive(p, name, ratio, shift=0):
    """get_to_dedup_ratio on device and model, then everything a reader sees of the new file."""
    unique = [ln for _, ln in bm.unique_spans(p.m.files[name])]
    new = p.fs.get_to_dedup_ratio(name, ratio)
    assert new == bm.get_to_dedup_ratio(p.m, name, ratio) == bm.name_of(name, ratio)
    hm = p.open(new, readonly=True)
    want = p.check_file(hm, shift)  # stat, read_complete bytes and spans (true offsets), hashes
    spans = p.m._spans(hm[1])
    assert len(spans) == len(bm.closed_form(unique, ratio))
    _, r = bm.sizes(unique, ratio)
    for i in sorted({r, 2 * r, len(spans) // 3, len(spans) // 2, len(spans) - 1}):  # r: the first repeat boundary
        if 0 < i < len(spans):
            p.pread(hm, max(spans[i].offset - 3, 0), 9, shift=1)
    return hm, want


# ---- 1. dedup-ratio files --------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["none", "one", "two", "wrap", "plain"])
def test_derived_files_match_the_model(spec):
    import chunkfs_amd as c
    p = Pair(c)
    _build(p, "a", SPECS[spec])
    # 1.0: R = U, one exact cycle; 3.99, 4.0, 7.3: q >= 3 full cycles and a partial one; "wrap" has the empty
    # entry at the cycle wrap; 25.0 on "wrap" repeats only the empty entry and is refused below.
    ratios = [1.0, 1.005, 1.5, 2.0, 3.99, 4.0, 7.3] + ([25.0] if spec != "wrap" else [])
    for k, ratio in enumerate(ratios):
        hm, want = _derive(p, "a", ratio, shift=k % 3)
        if spec in ("none", "one"):
            assert want.size == 0 and p.fs.stat(hm[0])["spans"] == 0  # U = 0
    assert sorted(p.fs.list_files()) == p.m.list()


def test_cycle_counts_of_the_hand_made_files():
    """The cases above are the ones the issue names: pinned here so that a change of SPEC_* cannot lose them."""
    wrap = [ln for _, ln in SPEC_WRAP[:-1]]
    uniq_wrap = [0, 40, 60, 100, 1, 99, 77, 23]
    uniq_plain = [40, 60, 100, 1, 99, 0, 77, 23, 50]
    assert sum(wrap) - 40 - 60 == sum(uniq_wrap) == 400
    partial = 0
    for uniq, ratio in ((uniq_wrap, 3.99), (uniq_wrap, 4.0), (uniq_wrap, 7.3), (uniq_plain, 3.99), (uniq_plain, 7.3)):
        total, r = bm.sizes(uniq, ratio)
        assert total // sum(uniq[:r]) >= 3  # q >= 3 full cycles
        partial += total % sum(uniq[:r]) > 0
    assert partial >= 3  # ... and a partial one; the others end on a wrap, where the empty entry is taken again
    assert bm.sizes(uniq_wrap, 1.0)[1] == len(uniq_wrap)
    assert bm.closed_form(uniq_wrap, 1.0) == list(range(8)) + [0]  # the empty entry at the wrap is taken again
    assert bm.never_ends(uniq_wrap, 25.0) and not bm.never_ends(uniq_plain, 25.0)


def test_refusals_change_nothing():
    import chunkfs_amd as c
    p = Pair(c)
    _build(p, "a", SPEC_WRAP)
    _derive(p, "a", 2.0)
    files, stats = p.fs.list_files(), p.fs.store.stats()
    for ratio in (25.0, 0.99, math.nan, math.inf):  # 25.0: R = 1 and the repeating span is empty (C == 0)
        with pytest.raises(c.CdcError) as ei:
            p.fs.get_to_dedup_ratio("a", ratio)
        assert _code(ei) == EINVAL, ratio
        with pytest.raises(fm.ModelError) as mi:
            bm.get_to_dedup_ratio(p.m, "a", ratio)
        assert mi.value.code == EINVAL
    with pytest.raises(c.CdcError) as ei:
        p.fs.get_to_dedup_ratio("missing", 2.0)
    assert _code(ei) == ENOTFOUND
    assert p.fs.list_files() == files == ["a", "a.2.00"] and p.fs.store.stats() == stats
    p.check_file(p.open("a.2.00", readonly=True))
    # too small a name buffer: the size it needs comes back, nothing is written, the file exists all the same
    L = c._lib.lib()
    buf = ctypes.create_string_buffer(b"\xA5" * 8, 8)
    assert L.cdc_files_get_to_dedup_ratio(p.fs._h, b"a", 1.5, buf, 6, None) == len("a.1.50") + 1
    assert buf.raw == b"\xA5" * 8
    assert bm.get_to_dedup_ratio(p.m, "a", 1.5) == "a.1.50"
    p.check_file(p.open("a.1.50", readonly=True))
    buf = ctypes.create_string_buffer(b"\xA5" * 8, 8)
    assert L.cdc_files_get_to_dedup_ratio(p.fs._h, b"a", 1.5, buf, 7, None) == 7 and buf.raw == b"a.1.50\0\xA5"


def test_replacement_derived_of_derived_and_clear():
    import chunkfs_amd as c
    p = Pair(c)
    w = _build(p, "a", SPEC_PLAIN)
    first, _ = _derive(p, "a", 2.0)
    n_first = p.fs.stat(first[0])["spans"]
    p.append(w, DATA, [(5, 30), (450, 10)])  # the source grows: the next call derives a different file
    second, _ = _derive(p, "a", 2.0)
    assert p.fs.stat(second[0])["spans"] != n_first
    p.check_file(first)  # a handle opened on the replaced file sees the new one
    _, want = _derive(p, "a.2.00", 1.5, shift=2)  # a call on the derived file itself
    assert sorted(p.fs.list_files()) == ["a", "a.2.00", "a.2.00.1.50"] and want.size > 0
    p.fs.store.clear()  # the source is under a stale store epoch
    with pytest.raises(c.CdcError) as ei:
        p.fs.get_to_dedup_ratio("a", 2.0)
    assert _code(ei) == ENOTFOUND and sorted(p.fs.list_files()) == ["a", "a.2.00", "a.2.00.1.50"]
    p.fs.clear_database()
    with pytest.raises(c.CdcError) as ei:
        p.fs.get_to_dedup_ratio("a", 2.0)
    assert _code(ei) == ENOTFOUND and p.fs.list_files() == []


def _many_spans(n=5001, seed=5):
    """n spans of 1..40 bytes tiling random data: about n unique digests."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 41, size=n).astype(np.uint64)
    data = oracle.splitmix64_bytes(int(lengths.sum()), seed)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64)
    return data, np.stack([offs, lengths], axis=1)


def test_five_thousand_unique_spans_at_ratio_three():
    import chunkfs_amd as c
    data, chunks = _many_spans()
    p = Pair(c, max_chunks=1 << 13)
    _build(p, "big", chunks, data)
    hm, want = _derive(p, "big", 3.0, shift=1)
    spans = p.fs.stat(hm[0])["spans"]
    assert spans > 3 * 2048 and spans > 64  # several scan blocks; the new table grew past its first 64 entries
    unique = [ln for _, ln in bm.unique_spans(p.m.files["big"])]
    total, r = bm.sizes(unique, 3.0)
    repeating = want.size - sum(unique[r:])
    assert total - 40 < repeating <= total  # the repeating part stops within one span (at most 40 bytes) of the total


class BenchScrubPair(ScrubPair):
    """ScrubPair with the scrubbers this suite needs: COPY, and RECHUNK with a 64-byte FSChunker."""

    def __init__(self, c, kind, **kw):
        self.c, self.kind, self.seg = c, kind, 4096
        scrubber = c.CopyScrubber() if kind == "copy" else c.RechunkScrubber(c.FSChunker(64))
        self.fs = c.FileSystem.new_with_scrubber(scrubber, max_chunks=1 << 12, arena_bytes=4 * MB,
                                                 target_max_chunks=1 << 14, target_arena_bytes=4 * MB, seg_size=4096)
        self.m = scm.FileSystem(seg_size=4096)

    def scrub(self):
        got = self.fs.scrub()
        ms = self.m.store
        want = ms.scrub_copy() if self.kind == "copy" else ms.scrub_rechunk(
            lambda b: oracle.fixed(len(b), 64) if len(b) else [])
        assert (got.processed_data, got.data_left) == (want.processed_data, want.data_left)
        return got


@pytest.mark.parametrize("kind", ["copy", "fixed64"])
@pytest.mark.parametrize("order", ["derive_then_scrub", "scrub_then_derive"])
def test_scrub_ordering(order, kind):
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(3000, 9)
    chunks = [(0, 0), (0, 300), (300, 700), (0, 300), (1000, 65), (1065, 935), (300, 700), (2000, 1000), (0, 1)]
    p = BenchScrubPair(c, kind)
    _build(p, "f", chunks, data)
    if order == "derive_then_scrub":
        _derive(p, "f", 2.5)
        p.scrub()
    else:
        p.scrub()
        _derive(p, "f", 2.5, shift=1)
    assert p.fs.store.scrub_stats()["chunk_containers"] == 0
    for name in ("f", "f.2.50"):
        p.check_reads(name)
    hm = p.open("f.2.50", readonly=True)
    for off, ln in ((290, 80), (999, 70), (1063, 200), (0, 5000)):
        p.pread(hm, off, ln, shift=1)
    _derive(p, "f.2.50", 1.5)  # and once more in the scrubbed state
    p.check_store()


# ---- 2. verify -------------------------------------------------------------------------------
class DeviceData:
    """A host array in HBM whose first byte sits at address = `mis` mod 16, with room for one more byte."""

    def __init__(self, arr, mis):
        import torch
        self.t = torch.zeros(arr.size + 64, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.off, self.n = 16 + mis, arr.size
        self.t[self.off:self.off + arr.size] = torch.from_numpy(np.array(arr, dtype=np.uint8)).cuda()
        torch.cuda.synchronize()

    @property
    def ptr(self):
        return self.t.data_ptr() + self.off

    def flip(self, pos):
        import torch
        self.t[self.off + pos] ^= 0xFF
        torch.cuda.synchronize()


def _verify_flips(p, hm, want, positions, misalignments):
    """One flipped dataset byte per call: first_diff must be exactly that offset."""
    for mis in misalignments:
        d = DeviceData(want, mis)
        assert p.fs.verify_device(hm[0], d.ptr, want.size) == (True, None) == bm.verify(want, want)
        for pos in positions(d.ptr):
            d.flip(pos)
            assert p.fs.verify_device(hm[0], d.ptr, want.size) == (False, pos), (mis, pos)
            d.flip(pos)
        assert p.fs.verify_device(hm[0], d.ptr, want.size) == (True, None)


def _edges(big, size, more=()):
    """The places of one flipped byte, for a dataset at address ptr; `big` is a span of more than two tiles."""
    assert big.len > 3 * 4096

    def positions(ptr):
        b, e = big.offset, big.offset + big.len
        tile = b - ((ptr + b) & 15) + 2 * 4096  # tiles are aligned in dataset space: the third tile of the piece
        return [0, size - 1,               # offset 0, the last byte
                b - 1, b, b + 1,           # a span boundary +-1
                tile - 1, tile, tile + 1,  # a 4096-byte tile boundary +-1
                b + 2, e - 2] + list(more)  # inside the ragged head and tail of the piece
    return positions


def _hand_made_300k(p):
    base = [1, 15, 16, 17, 0, 4095, 4096, 4097, 33, 20000, 7, 64, 0, 1000, 12289]
    lengths = np.array(base * 7, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64)
    tiling = np.stack([offs, lengths], axis=1)
    chunks = np.concatenate([tiling, tiling[[9, 5, 4, 24]]])  # duplicate spans: 20000 bytes, 4095, empty, 20000
    data = oracle.splitmix64_bytes(int(lengths.sum()), 31)
    w = _build(p, "v", chunks, data)
    hm = p.open("v", readonly=True)
    want = p.m.read_complete(hm[1])
    assert want.size == int(lengths.sum()) + 20000 + 4095 + 20000 > 300_000
    return w, hm, want


def test_verify_hand_made_spans_every_edge():
    import chunkfs_amd as c
    p = Pair(c)
    _, hm, want = _hand_made_300k(p)
    spans = p.m._spans(hm[1])
    big = spans[9]  # the first 20000-byte span; offset 0 is a 1-byte span
    assert big.len == 20000 and spans[0].len == 1 and spans[4].len == 0
    more = [spans[4].offset - 1, spans[4].offset, spans[5].offset + 4094]  # around an empty span; a 4095-byte span's end
    _verify_flips(p, hm, want, _edges(big, want.size, more), (0, 1, 7, 15))
    d = DeviceData(want, 7)
    for pos in (big.offset + 5000, 70, want.size - 1):  # two and three flips: the smallest offset wins
        d.flip(pos)
    assert p.fs.verify_device(hm[0], d.ptr, want.size) == (False, 70)
    d.flip(70)
    assert p.fs.verify_device(hm[0], d.ptr, want.size) == (False, big.offset + 5000)


def test_verify_sizes_empty_and_stale():
    import chunkfs_amd as c
    p = Pair(c)
    _, hm, want = _hand_made_300k(p)
    for mis in (0, 3):
        d = DeviceData(want, mis)
        n = want.size
        assert p.fs.verify_device(hm[0], d.ptr, n - 1) == (False, n - 1) == bm.verify(want, want[:-1])
        assert p.fs.verify_device(hm[0], d.ptr, n + 1) == (False, n)  # one byte longer: the room DeviceData leaves
        d.flip(n - 1)  # past a shorter dataset's end: not compared
        assert p.fs.verify_device(hm[0], d.ptr, n - 1) == (False, n - 1)
        d.flip(100)  # a difference inside the common prefix comes first
        assert p.fs.verify_device(hm[0], d.ptr, n - 1) == (False, 100)
    e = p.create("empty")
    assert p.fs.verify_device(e[0], None, 0) == (True, None)
    assert p.fs.verify_device(e[0], d.ptr, 5) == (False, 0)
    assert p.fs.verify_device(hm[0], None, 0) == (False, 0)
    with pytest.raises(c.CdcError) as ei:
        p.fs.verify_device(hm[0], None, 5)
    assert _code(ei) == EINVAL
    p.fs.store.clear()  # a stale epoch
    with pytest.raises(c.CdcError) as ei:
        p.fs.verify_device(hm[0], d.ptr, want.size)
    assert _code(ei) == ENOTFOUND


def test_verify_three_mib_fastcdc_write():
    import chunkfs_amd as c
    data = oracle.splitmix64_bytes(3 * MB, 17)
    p = Pair(c)
    w = p.create("w", c.FastChunker(c.SizeParams(*FAST)))
    lengths = oracle.fastcdc(data, *FAST)[:, 1]
    p.write(w, data, lengths)
    big = next(sp for sp in p.m._spans(w[1])[50:] if sp.len > 3 * 4096)  # a chunk in the middle of the file
    _verify_flips(p, w, data, _edges(big, data.size, [2 * MB + 12345]), (0, 1, 7, 15))


@pytest.mark.parametrize("kind", ["copy", "fixed64"])
def test_verify_after_scrub(kind):
    import chunkfs_amd as c
    p = BenchScrubPair(c, kind)
    _, hm, want = _hand_made_300k(p)
    p.scrub()
    big = p.m._spans(hm[1])[9]

    b = big.offset
    more = [b + 63, b + 64, b + 65, b + 127, b + 19999]  # 64-byte sub-chunk boundaries +-1 inside a container
    _verify_flips(p, hm, want, _edges(big, want.size, more), (0, 1, 7, 15))
    d = DeviceData(want, 5)
    assert p.fs.verify_device(hm[0], d.ptr, want.size - 1) == (False, want.size - 1)
    p.fs.target.clear()  # the keys point into a cleared target
    with pytest.raises(c.CdcError) as ei:
        p.fs.verify_device(hm[0], d.ptr, want.size)
    assert _code(ei) == ENOTFOUND


# ---- 3. size distribution --------------------------------------------------------------------
def _check_distribution(c, fs, model_lengths, extra=()):
    """ChunkStore.size_distribution against the model over storage_iterator()'s lengths."""
    lengths = sorted(ln for _, _, ln, _ in fs.storage_iterator())
    assert lengths == sorted(model_lengths)
    top = max(lengths) if lengths else 0
    for adj in (1, 1000, 4096, top + 1) + tuple(extra):
        want = bm.size_distribution(lengths, adj)
        got = fs.store.size_distribution(adj)
        assert got == want, adj
        assert list(got) == sorted(got)  # ascending size order
    if lengths:
        assert fs.store.size_distribution(top + 1) == {0: len(lengths)}  # one above every length: the single bin 0
    with pytest.raises(c.CdcError) as ei:
        fs.store.size_distribution(0)
    assert _code(ei) == EINVAL


def test_size_distribution_hand_made_and_cap():
    import torch
    import chunkfs_amd as c
    p = Pair(c)
    _, hm, _ = _hand_made_300k(p)  # lengths 0 .. 20000, a zero-length container among them
    lengths = [len(b) for b in p.m.store.db.values()]
    assert 0 in lengths
    _check_distribution(c, p.fs, lengths, extra=(7, 20000))
    # cap one too small: the count comes back and nothing is written; with room, nothing past the count
    want = bm.size_distribution(lengths, 1000)
    n = len(want)
    L, P = c._lib.lib(), ctypes.c_void_p
    sizes = torch.full((n + 3,), -1, dtype=torch.int64, device="cuda")
    counts = torch.full((n + 3,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h = p.fs.store._h
    assert L.cdc_store_size_distribution_device(h, 1000, P(sizes.data_ptr()), P(counts.data_ptr()), n - 1, None) == n
    assert (sizes.cpu().numpy() == -1).all() and (counts.cpu().numpy() == -1).all()
    assert L.cdc_store_size_distribution_device(h, 1000, P(sizes.data_ptr()), P(counts.data_ptr()), n, None) == n
    s, k = sizes.cpu().numpy(), counts.cpu().numpy()
    assert dict(zip(s[:n].tolist(), k[:n].tolist())) == want and (s[n:] == -1).all() and (k[n:] == -1).all()
    p.fs.clear_database()
    assert p.fs.store.size_distribution(4096) == {} == bm.size_distribution([], 4096)


def test_size_distribution_many_and_equal_containers():
    import chunkfs_amd as c
    data, chunks = _many_spans()
    p = Pair(c, max_chunks=1 << 13)
    _build(p, "big", chunks, data)  # more than 2048 containers, lengths 1..40
    lengths = [len(b) for b in p.m.store.db.values()]
    assert len(lengths) > 2048
    _check_distribution(c, p.fs, lengths, extra=(3, 16))
    # FSChunker: every container has one length, every lane of a wave hits one bin
    p = Pair(c)
    flat = oracle.splitmix64_bytes(MB, 3)
    w = p.create("flat", c.FSChunker(4096))
    p.write(w, flat, oracle.fixed(flat.size, 4096)[:, 1])
    assert p.fs.store.size_distribution(4096) == {4096: 256} == p.fs.store.size_distribution(1)
    assert p.fs.store.size_distribution(4097) == {0: 256}
    _check_distribution(c, p.fs, [4096] * 256)


@pytest.mark.parametrize("kind", ["copy", "fixed64"])
def test_size_distribution_counts_both_kinds(kind):
    import chunkfs_amd as c
    p = BenchScrubPair(c, kind)
    _hand_made_300k(p)
    before = p.fs.store.size_distribution(1000)
    p.scrub()
    late = oracle.splitmix64_bytes(5000, 8)
    _build(p, "late", [(0, 1234), (1234, 3766)], late)  # chunk-kind containers beside the target-kind ones
    kinds = {k for _, k, _, _ in p.fs.storage_iterator()}
    assert kinds == {"chunk", "target"}
    lengths = [v[1] for v in p.m.store.iterator().values()]
    _check_distribution(c, p.fs, lengths)
    after = p.fs.store.size_distribution(1000)
    assert sum(after.values()) == sum(before.values()) + 2 and after[1000] == before.get(1000, 0) + 1


# ---- 4. the fixture ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """2 MiB on disk whose second MiB repeats the first: the dedup ratio is not 1."""
    from chunkfs_amd.bench import Dataset
    half = oracle.splitmix64_bytes(MB, 11)
    path = tmp_path_factory.mktemp("bench") / "dataset.bin"
    path.write_bytes(half.tobytes() * 2)
    return Dataset(str(path), "twice")


def _fixture(c):
    from chunkfs_amd.bench import CDCFixture
    return CDCFixture(max_chunks=1 << 12, arena_bytes=16 * MB)


def _model_ratio(data, lengths):
    m = sm.Model()
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64)
    m.put(data, np.stack([offs, np.asarray(lengths, dtype=np.uint64)], axis=1))
    st = m.stats()
    return st["bytes_written"] / st["unique_bytes"], st


def test_fixture_measure_fields(dataset):
    import chunkfs_amd as c
    fx = _fixture(c)
    ch = c.FastChunker(c.SizeParams(*FAST))
    r = fx.measure(dataset, ch)
    data = np.fromfile(dataset.path, dtype=np.uint8)
    want_ratio, st = _model_ratio(data, oracle.fastcdc(data, *FAST)[:, 1])
    assert want_ratio > 1.5
    assert (r.size, r.name, r.path, r.chunker) == (2 * MB, "twice", dataset.path, repr(ch))
    assert r.chunk_count == st["unique_chunks"] == fx.chunk_count() == len(fx.fs.storage_iterator())
    assert r.dedup_ratio == fx.fs.cdc_dedup_ratio() == want_ratio
    assert r.full_dedup_ratio == fx.fs.full_cdc_dedup_ratio()
    assert r.avg_chunk_size == fx.fs.average_chunk_size() == st["unique_bytes"] // st["unique_chunks"]
    m, t = r.measurement, r.throughput
    assert min(m.write_time, m.read_time, m.chunk_time, m.hash_time) > 0
    assert m.chunk_time + m.hash_time < m.write_time  # the two are parts of the write
    assert (t.write, t.read, t.chunk, t.hash) == (2 / m.write_time, 2 / m.read_time, 2 / m.chunk_time,
                                                  2 / m.hash_time)
    assert fx.fs.file_exists(r.file_name) and len(r.file_name) == 36  # a uuid4
    lengths = [ln for _, _, ln, _ in fx.fs.storage_iterator()]
    assert fx.size_distribution(4096) == bm.size_distribution(lengths, 4096)


def test_fixture_multi_repeated_and_dedup_ratio(dataset):
    import chunkfs_amd as c
    fx = _fixture(c)
    ch = c.FastChunker(c.SizeParams(*FAST))
    with dataset.open() as f:
        fx.fill_with(f, ch)  # what measure_multi must clear first
    multi = fx.measure_multi(dataset, ch, 3)
    assert len({r.chunk_count for r in multi}) == 1 and len({r.dedup_ratio for r in multi}) == 1
    assert len({r.file_name for r in multi}) == 3 and fx.fs.list_files() == [multi[-1].file_name]
    rep = fx.measure_repeated(dataset, ch, 3)
    assert rep[0].dedup_ratio == multi[0].dedup_ratio
    assert rep[0].dedup_ratio < rep[1].dedup_ratio < rep[2].dedup_ratio  # nothing is cleared between the runs
    assert rep[1].dedup_ratio == 2 * rep[0].dedup_ratio and len(fx.fs.list_files()) == 3
    assert {r.chunk_count for r in rep} == {multi[0].chunk_count}
    d = fx.dedup_ratio(dataset, ch)
    assert (d.name, d.dedup_ratio) == ("twice", multi[0].dedup_ratio) and len(fx.fs.list_files()) == 1


def test_fixture_verify_names_the_first_changed_byte(dataset, tmp_path):
    import chunkfs_amd as c
    from chunkfs_amd.bench import Dataset, VerifyError
    path = tmp_path / "copy.bin"
    raw = bytearray(open(dataset.path, "rb").read())
    path.write_bytes(raw)
    ds = Dataset(str(path), "copy")
    fx = _fixture(c)
    r = fx.measure(ds, c.FSChunker(4096))
    assert fx.verify(ds, r.file_name) > 0
    for pos in (MB + 4097, 5):  # the dataset file changes after the write
        raw[pos] ^= 1
        path.write_bytes(raw)
        with pytest.raises(VerifyError, match="contents of dataset and written file are different") as ei:
            fx.verify(ds, r.file_name)
        assert ei.value.first_diff == pos and str(pos) in str(ei.value)
    path.write_bytes(raw[:-1])
    with pytest.raises(VerifyError, match="dataset size and size of written file are different"):
        fx.verify(Dataset(str(path), "short"), r.file_name)


def test_fixture_round_trip_through_a_derived_file(dataset, tmp_path):
    import chunkfs_amd as c
    from chunkfs_amd.bench import Dataset
    fx = _fixture(c)
    ch = c.FastChunker(c.SizeParams(*FAST))
    data = np.fromfile(dataset.path, dtype=np.uint8)
    h = fx.fs.create_file("f", ch)
    with dataset.open() as f:
        fx.fs.write_from_stream(h, f)
    fx.fs.close_file(h)
    name = fx.fs.get_to_dedup_ratio("f", 4.0)
    assert name == "f.4.00"
    # the model of the same file: the oracle's chunks of the dataset, derived by the transcription
    files = fm.Files()
    files.append_lengths(files.create("f"), data, oracle.fastcdc(data, *FAST)[:, 1])
    assert bm.get_to_dedup_ratio(files, "f", 4.0) == name
    want = files.read_complete(files.open(name))
    out = tmp_path / "derived.bin"
    fx.fs.write_file_to_disk(name, str(out))
    got = np.fromfile(str(out), dtype=np.uint8)
    assert got.size == want.size and (got == want).all()
    r = fx.dedup_ratio(Dataset(str(out), "derived"), ch)  # clears, writes, verifies
    want_ratio, _ = _model_ratio(want, oracle.fastcdc(want, *FAST)[:, 1])
    assert r.dedup_ratio == want_ratio and want_ratio > 3
