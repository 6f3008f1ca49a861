"""GPU suite of cdc_file_splice_device (include/chunkfs_amd.h, "Editing a file in
place") against the model of tests/splice_model.py.  After every call: the span
list, the digests, the bytes, stat and every stats field equal the model's;
window_bytes is compared as <= the model's restart-from-off[i0] figure.  The
cases are the ones tests/test_splice_model.py proves to reach the hard paths."""
import ctypes
import os

import numpy as np
import pytest

import gc_model as gm
import splice_model as spm
import store_model as sm
from test_gpu_files import _code
from test_gpu_gc import GcPair

pytestmark = pytest.mark.gpu
MB = 1 << 20
EXACT = ("first_span", "spans_removed", "spans_inserted", "resync_offset", "size_before", "size_after", "bytes_new",
         "rounds")


class SPair(GcPair):
    """The device layer and the model, spliced side by side."""

    def __init__(self, c, name, max_chunks=1 << 13, arena=8 * MB, fs=None):
        super().__init__(c, max_chunks=max_chunks, arena=arena, fs=fs)
        self.name, self.chunker = name, spm.make_chunker(c, name)

    def new_file(self, fname, data=None, chunks=None):
        """A file written in one call (chunks: what the model chunker gives for it)."""
        hm = self.create(fname, self.chunker)
        if data is not None and data.size:
            chunks = spm.chunk(self.name, data) if chunks is None else chunks
            assert self.fs.write_to_file(hm[0], data) == len(chunks)
            self.m.append(hm[1], data, chunks)
            self.seen.update(self.m.hashes(hm[1]))
        return hm

    def splice(self, hm, offset, rem, ins):
        h, mh = hm
        got = self.fs.splice(h, offset, rem, ins).as_dict()
        want = spm.splice(self.m, mh, self.name, offset, rem, ins)
        self.seen.update(self.m.hashes(mh))
        assert {k: got[k] for k in EXACT} == {k: want[k] for k in EXACT}, (got, want)
        assert 0 < got["window_bytes"] <= want["window_bytes"] or want["window_bytes"] == got["window_bytes"] == 0
        self.check_file(hm, shift=3)  # stat, read_complete with its spans, hashes
        return got


def slots_of(c, fs, h):
    n = fs.stat(h)["spans"]
    s, loc = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint64 * max(n, 1))()
    assert c._lib.lib().cdc_debug_file_slots(h._fh, s, loc, n) == n
    return list(s)[:n], list(loc)[:n]


# ---- every chunker, every kind of edit, three places ----------------------------------------
@pytest.mark.parametrize("name", list(spm.CHUNKERS))
def test_random_edits(name):
    import chunkfs_amd as c
    data, chunks = spm.base(name)
    p = SPair(c, name)
    for label, offset, rem, ins in spm.random_cases(name):
        hm = p.new_file(label, data, chunks)
        p.splice(hm, offset, rem, ins)
    sm.assert_stats(p.fs.store, p.m.store)


@pytest.mark.parametrize("name", ["fast", "ae", "fixed"])
def test_edges(name):
    import chunkfs_amd as c
    data, chunks = spm.base(name)
    p = SPair(c, name)
    for label, (offset, rem, ins) in spm.edge_cases(name).items():
        hm = p.new_file(label, data, chunks)
        p.splice(hm, offset, rem, ins)
        if label in ("truncate_to_0", "delete_all"):
            assert p.fs.stat(hm[0])["spans"] == 0
            p.splice(hm, 0, 0, spm.rand(9, 700))  # and the emptied file takes bytes again
    sm.assert_stats(p.fs.store, p.m.store)


@pytest.mark.parametrize("name", list(spm.CHUNKERS))
def test_splice_into_an_empty_file_equals_a_write(name):
    import chunkfs_amd as c
    p = SPair(c, name)
    data = spm.rand(4001, 20000)
    hm = p.new_file("spliced")
    got = p.splice(hm, 0, 0, data)
    twin = p.new_file("written", data)
    assert spm.table(p.m, hm[1]) == spm.table(p.m, twin[1])
    assert [bytes(d) for d in p.fs.hashes(hm[0])] == [bytes(d) for d in p.fs.hashes(twin[0])]
    assert got["spans_inserted"] == p.fs.stat(twin[0])["spans"]
    assert p.fs.splice(hm[0], 5, 0, None).as_dict()["spans_inserted"] == 0  # nothing to do: touches nothing
    p.check_file(hm)


def test_zero_length_spans_at_the_resync_offset():
    import chunkfs_amd as c
    name = "fast"
    data, chunks = spm.base(name, seed=5, n=32 << 10)
    i = 20
    offset = int(chunks[i][0]) + int(chunks[i][1]) // 2
    probe = gm.Files()
    ph = probe.create("f")
    probe.append(ph, data, chunks)
    s = spm.splice(probe, ph, name, offset, 1, spm.rand(5001, 1))
    j = s["first_span"] + s["spans_removed"]
    holes = np.concatenate([chunks[:j], [[chunks[j][0], 0]] * 2, chunks[j:]])
    p = SPair(c, name)
    hm = p.create("f", p.chunker)
    p.append(hm, data, holes)  # cdc_file_append_device
    got = p.splice(hm, offset, 1, spm.rand(5001, 1))
    assert got["first_span"] + got["spans_removed"] == j and got["resync_offset"] == int(chunks[j][0])
    p.check_reads("f")


# ---- several rounds ------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(spm.round_cases()))
def test_rounds(label):
    import chunkfs_amd as c
    name, data, offset, rem, ins = spm.round_cases()[label]
    p = SPair(c, name)
    hm = p.new_file("f", data)
    got = p.splice(hm, offset, rem, ins)
    if label == "fixed_insert_512":
        assert got["rounds"] == 1
    else:
        assert got["rounds"] >= 3 and got["resync_offset"] == got["size_after"]
    p.check_reads("f")


# ---- table paths ---------------------------------------------------------------------------
def test_patch_growth_shrink_and_the_pool():
    import chunkfs_amd as c
    name = "fast"
    p = SPair(c, name)
    data = spm.rand(6001, 16 << 10)
    chunks = spm.chunk(name, data)
    assert 40 < len(chunks) < 64
    hm = p.new_file("f", data, chunks)
    # the in-place patch: equal counts, delta == 0
    mid = int(chunks[len(chunks) // 2][0]) + 20
    got = p.splice(hm, mid, 1, spm.rand(6002, 1))
    assert got["spans_inserted"] == got["spans_removed"] and got["size_after"] == got["size_before"]
    slots, locs = slots_of(c, p.fs, hm[0])
    got = p.splice(hm, mid, 1, spm.rand(6003, 1))  # again: everything outside the replaced entries stays
    s2, l2 = slots_of(c, p.fs, hm[0])
    a, b = got["first_span"], got["first_span"] + got["spans_inserted"]
    assert (s2[:a], l2[:a], s2[b:], l2[b:]) == (slots[:a], locs[:a], slots[b:], locs[b:])
    # growth across a capacity doubling
    before = p.fs.stat(hm[0])["spans"]
    p.splice(hm, 3000, 0, spm.rand(6004, 12000))
    assert before < 64 < p.fs.stat(hm[0])["spans"] <= 128
    # shrink
    p.splice(hm, 1000, 20000, None)
    assert p.fs.stat(hm[0])["spans"] < 64
    p.check_reads("f")
    # the pool: tables go back and come out again
    lib = c._lib.lib()
    p.splice(hm, 2000, 0, spm.rand(6100, 300))
    p.splice(hm, 2000, 300, None)
    blocks = lib.cdc_debug_files_table_blocks(p.fs._h)
    for k in range(25):
        p.splice(hm, 2000 + k, 0, spm.rand(6101 + k, 300))
        p.splice(hm, 2000 + k, 300, None)
    assert lib.cdc_debug_files_table_blocks(p.fs._h) == blocks
    sm.assert_stats(p.fs.store, p.m.store)


def test_spans_outside_the_edit_keep_digest_slot_and_location():
    import chunkfs_amd as c
    name = "rabin"
    p = SPair(c, name)
    hm = p.create("f", p.chunker)
    parts = [spm.rand(7001 + k, 20000 + 777 * k) for k in range(3)]
    for part in parts:  # three calls: the cuts at the seams are not the chunker's own
        ch = spm.chunk(name, part)
        assert p.fs.write_to_file(hm[0], part) == len(ch)
        p.m.append(hm[1], part, ch)
    old_table, (slots, locs) = spm.table(p.m, hm[1]), slots_of(c, p.fs, hm[0])
    got = p.splice(hm, 30000, 10, spm.rand(7100, 123))
    i0, j, m = got["first_span"], got["first_span"] + got["spans_removed"], got["spans_inserted"]
    assert 0 < i0 and j < len(old_table) and got["resync_offset"] < got["size_after"]
    new_table, (s2, l2) = spm.table(p.m, hm[1]), slots_of(c, p.fs, hm[0])
    assert (s2[:i0], l2[:i0]) == (slots[:i0], locs[:i0]) and (s2[i0 + m:], l2[i0 + m:]) == (slots[j:], locs[j:])
    assert new_table[:i0] == old_table[:i0]
    assert [(o - 113, ln, d) for o, ln, d in new_table[i0 + m:]] == old_table[j:]
    p.check_reads("f")


# ---- a script of edits, then collect --------------------------------------------------------
@pytest.mark.parametrize("name", ["fast", "seq"])
def test_twenty_edits_then_collect(name):
    import chunkfs_amd as c
    p = SPair(c, name, max_chunks=1 << 12)
    data = spm.rand(8001, 64 << 10)
    hm = p.new_file("f", data)
    p.open_files["f"] = hm
    for k, (offset, rem, ins) in enumerate(spm.random_script(8002, data.size)):
        p.splice(hm, offset, rem, spm.rand(8100 + k, ins) if ins else None)
    sm.assert_stats(p.fs.store, p.m.store)
    r = p.collect()  # the replaced spans' containers are ordinary garbage
    assert r["containers_after"] < r["containers_before"]
    p.check_all()
    # a fresh layer holding the final content, written span for span by the model's table
    final = p.m.read_complete(hm[1])
    fresh = GcPair(c)
    fh = fresh.create("f")
    fresh.append(fh, final, [[o, ln] for o, ln, _ in spm.table(p.m, hm[1])])
    a, b = p.fs.store.stats(), fresh.fs.store.stats()
    assert {k: a[k] for k in ("unique_chunks", "unique_bytes", "arena_used")} == \
        {k: b[k] for k in ("unique_chunks", "unique_bytes", "arena_used")}
    assert r["containers_after"] == b["unique_chunks"]


# ---- refusals -----------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import chunkfs_amd as c
    L = c._lib.lib()
    name = "fast"
    p = SPair(c, name)
    data = spm.rand(9001, 30000)
    hm = p.new_file("f", data)
    ro = p.open("f", readonly=True)
    ins = sm.dev(spm.rand(9002, 100))
    st = c._lib.cdc_splice_stats_t(rounds=77)
    ch, fh = p.chunker._h, hm[0]._fh

    def raw(fh_, ch_, offset, rem, ptr, n):
        return L.cdc_file_splice_device(fh_, ch_, offset, rem, ptr, n, ctypes.byref(st), None)

    def state():
        return (p.fs.stat(hm[0])["size"], p.fs.stat(hm[0])["spans"], p.fs.hashes(hm[0]).tobytes(),
                slots_of(c, p.fs, hm[0]), repr(p.fs.store.stats()))

    before = state()
    for args, code, words in (
            ((None, ch, 0, 0, ins.data_ptr(), 100), c._lib.CDC_EINVAL, b"NULL file handle"),
            ((fh, None, 0, 0, ins.data_ptr(), 100), c._lib.CDC_EINVAL, b"NULL chunker"),
            ((fh, ch, 0, 0, None, 100), c._lib.CDC_EINVAL, b"NULL data"),
            ((fh, ch, 30001, 0, ins.data_ptr(), 100), c._lib.CDC_EINVAL, b"offset 30001 is past"),
            ((fh, ch, 29000, 1001, ins.data_ptr(), 100), c._lib.CDC_EINVAL, b"offset + remove_len"),
            ((fh, ch, 1, 2 ** 64 - 1, None, 0), c._lib.CDC_EINVAL, b"offset + remove_len"),
            ((ro[0]._fh, ch, 0, 10, ins.data_ptr(), 100), c._lib.CDC_EPERM, b"read-only")):
        assert raw(*args) == code, args
        assert words in L.cdc_last_error(), (words, L.cdc_last_error())
        assert state() == before and st.rounds == 77
    with pytest.raises(c.CdcError) as e:  # the mirror refuses a read-only handle before it uploads
        p.fs.splice(ro[0], 0, 10, b"x")
    assert _code(e) == c._lib.CDC_EPERM
    with pytest.raises(c.CdcError) as e:
        p.fs.truncate(hm[0], 30001)
    assert _code(e) == c._lib.CDC_EINVAL
    assert raw(fh, ch, 7, 0, None, 0) == 0 and state() == before and st.rounds == 77  # nothing to do
    p.check_file(hm)
    # a removed file, and a file from another store epoch
    gone = p.new_file("gone", data)
    p.fs.remove_file("gone")
    p.m.remove("gone")
    before = state()  # the second file's write counted its chunks
    assert raw(gone[0]._fh, ch, 0, 1, None, 0) == c._lib.CDC_ENOTFOUND and b"no file named" in L.cdc_last_error()
    assert state() == before
    p.fs.store.clear()
    assert raw(fh, ch, 0, 1, None, 0) == c._lib.CDC_ENOTFOUND and b"cleared" in L.cdc_last_error()
    assert p.fs.stat(hm[0])["size"] == 30000


def test_a_scrubbed_store_is_not_supported():
    import chunkfs_amd as c
    fs = c.FileSystem.new_with_scrubber(c.CopyScrubber(), max_chunks=1 << 10, arena_bytes=MB,
                                        target_max_chunks=1 << 10, target_arena_bytes=MB)
    ch = spm.make_chunker(c, "fast")
    h = fs.create_file("f", ch)
    data = spm.rand(9101, 20000)
    fs.write_to_file(h, data)
    fs.splice(h, 100, 5, b"hello")  # a target is attached but nothing is scrubbed yet: allowed
    fs.scrub()
    before = (fs.stat(h)["size"], fs.stat(h)["spans"], fs.hashes(h).tobytes(), repr(fs.store.stats()))
    with pytest.raises(c.CdcError) as e:
        fs.splice(h, 100, 5, b"world")
    assert _code(e) == c._lib.CDC_ENOTSUP and "scrubbed" in str(e.value)
    assert (fs.stat(h)["size"], fs.stat(h)["spans"], fs.hashes(h).tobytes(), repr(fs.store.stats())) == before
    assert fs.read_file_complete(h).tobytes() == data[:100].tobytes() + b"hello" + data[105:].tobytes()


def test_a_refused_put_leaves_the_file_and_succeeds_after_collect():
    import chunkfs_amd as c
    name = "fast"
    p = SPair(c, name, max_chunks=1 << 10, arena=66000)
    a, b = p.new_file("a", spm.rand(9201, 30000)), p.new_file("b", spm.rand(9202, 30000))
    p.open_files.update(a=a, b=b)
    ins = spm.rand(9203, 5000)
    before = (p.fs.stat(a[0]), p.fs.hashes(a[0]).tobytes(), slots_of(c, p.fs, a[0]), p.fs.store.stats())
    with pytest.raises(c.CdcError) as e:
        p.fs.splice(a[0], 15000, 0, ins)  # the window's chunks do not fit beside the two files
    assert _code(e) == c._lib.CDC_ENOMEM
    assert (p.fs.stat(a[0]), p.fs.hashes(a[0]).tobytes(), slots_of(c, p.fs, a[0]), p.fs.store.stats()) == before
    p.check_file(a)
    p.remove("b")
    p.collect()
    p.splice(a, 15000, 0, ins)
    p.check_all()


# ---- two handles -------------------------------------------------------------------------------------
def test_a_reader_keeps_its_cursor_and_sees_the_new_bytes():
    import chunkfs_amd as c
    name = "ultra"
    p = SPair(c, name)
    data = spm.rand(9301, 40000)
    w = p.new_file("f", data)
    r = p.open("f", readonly=True)
    p.read_segment(r)
    cursor = p.fs.stat(r[0])["cursor"]
    assert 0 < cursor == r[1].offset
    p.splice(w, 100, 50, spm.rand(9302, 500))
    assert p.fs.stat(r[0])["cursor"] == cursor  # a number, as a POSIX descriptor's offset
    p.pread(r, 0, 2000)
    p.pread(r, cursor - 10, 300)
    assert p.fs.stat(r[0])["size"] == 40450


# ---- the thin forms and the C++ mirror ---------------------------------------------------------------
def test_pwrite_insert_delete_truncate():
    import chunkfs_amd as c
    import torch
    fs = c.FileSystem(max_chunks=1 << 10, arena_bytes=MB)
    ch = spm.make_chunker(c, "fixed")
    h = fs.create_file("f", ch)
    fs.write_to_file(h, bytes(range(200)) * 10)
    want = bytearray(bytes(range(200)) * 10)
    s = fs.pwrite(h, 1990, b"0123456789ABCDEF")  # overwrites ten bytes, extends by six
    want[1990:2000] = b"0123456789ABCDEF"
    assert (s.size_before, s.size_after) == (2000, 2006)
    fs.insert(h, 0, np.frombuffer(b"front", dtype=np.uint8))
    want[0:0] = b"front"
    fs.delete_range(h, 100, 1000)
    del want[100:1100]
    fs.pwrite(h, 50, torch.full((20,), 7, dtype=torch.uint8, device="cuda"))
    want[50:70] = bytes([7]) * 20
    fs.truncate(h, 600)
    del want[600:]
    assert fs.read_file_complete(h).tobytes() == bytes(want)
    assert fs.stat(h)["spans"] == 2 and fs.stat(h)["size"] == 600
    split = (ctypes.c_double * 5)()
    assert c._lib.lib().cdc_debug_splice_split(split, 5) == 5 and all(x >= 0 for x in split) and sum(split) > 0


def test_cpp_splice_example_runs():
    import subprocess
    from chunkfs_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "_build", "files_splice_example")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(root, "include"), "-isystem", os.path.join(rocm, "include"),
                    os.path.join(root, "examples", "files_splice_example.cpp"),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd", "-L", os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
                    "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "splice ok" in r.stdout
