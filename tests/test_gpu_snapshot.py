"""GPU suite of cdc_files_clone and cdc_files_diff_device (include/chunkfs_amd.h,
"Snapshots and diffs") against the model of tests/diff_model.py.  After every
diff the ranges and every stats field but `seconds` equal the model's,
bytes_compared exactly.  The cases are diff_model's, which
tests/test_diff_model.py proves to reach the paths they are named for; files are
a few hundred KiB at most, spans tens of bytes to a few KiB."""
import ctypes
import os

import numpy as np
import pytest

import diff_model as dm
import store_model as sm
from test_gpu_files import _code
from test_gpu_splice import SPair, slots_of

pytestmark = pytest.mark.gpu
MB = 1 << 20


class Driver:
    """diff_model's cases on the device layer, the model beside it: a handle is
    the pair (device handle, model handle) and every diff is compared."""

    def __init__(self, c, name="fast", max_chunks=1 << 13, arena=8 * MB, fs=None):
        self.c, self.name = c, name
        self.p = SPair(c, name, max_chunks=max_chunks, arena=arena, fs=fs)

    def file(self, fname, data, chunks=None):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if chunks is None:
            return self.p.new_file(fname, data)
        hm = self.p.create(fname, self.p.chunker)
        if len(chunks):
            self.p.append(hm, data, chunks)
        return hm

    def clone(self, src, dst):
        want = dm.clone(self.p.m, src, dst)
        assert self.p.fs.clone_file(src, dst) == want
        return self.p.open(dst, self.p.chunker)

    def splice(self, hm, offset, rem, ins):
        return self.p.splice(hm, offset, rem, ins)  # and the file against the model

    def diff(self, a, b, tables_only=False):
        got = self.p.fs.diff(a[0], b[0], tables_only=tables_only)
        want = dm.diff(self.p.m, a[1], b[1], tables_only)
        assert got.ranges.dtype == np.uint64 and got.ranges.shape == (got.n_ranges, 2)
        assert [tuple(r) for r in got.ranges.tolist()] == want["ranges"]
        for k in dm.STATS:
            assert getattr(got, k) == want[k], (k, getattr(got, k), want[k])
        assert got.seconds > 0
        return dict({k: getattr(got, k) for k in dm.STATS}, ranges=[tuple(r) for r in got.ranges.tolist()])


def raw_diff(c, fs, a, b, flags=0, d_ranges=None, cap=0, stats=None):
    return c._lib.lib().cdc_files_diff_device(a._fh, b._fh, flags, d_ranges, cap,
                                              ctypes.byref(stats) if stats is not None else None, None)


# ---- clone ---------------------------------------------------------------------------------
def test_a_clone_is_its_source_and_costs_the_store_nothing():
    import chunkfs_amd as c
    d = Driver(c)
    data = dm.rand(31, 96 << 10)
    a = d.file("a", data)
    before = d.p.fs.store.stats()
    b = d.clone("a", "b")
    assert d.p.fs.store.stats() == before
    sm.assert_stats(d.p.fs.store, d.p.m.store)
    assert slots_of(c, d.p.fs, a[0]) == slots_of(c, d.p.fs, b[0])
    assert (d.p.fs.hashes(a[0]) == d.p.fs.hashes(b[0])).all()
    sa, sb = d.p.fs.stat(a[0]), d.p.fs.stat(b[0])
    assert (sa["size"], sa["spans"]) == (sb["size"], sb["spans"]) == (data.size, len(d.p.m._spans(a[1])))
    assert (d.p.check_file(b, shift=3) == data).all() and (d.p.check_file(a) == data).all()
    assert d.p.fs.list_files() == ["a", "b"]
    # a derived file, built from a table too, leaves the stats alone as well: the clone is no exception
    d.p.fs.clone_file(d.p.fs.get_to_dedup_ratio("a", 2.0), "ratio_clone")
    assert d.p.fs.store.stats() == before


@pytest.mark.parametrize("edit_the", ["clone", "original"])
def test_an_edit_of_one_never_shows_through_the_other(edit_the):
    import chunkfs_amd as c
    d = Driver(c, "fixed")
    data = dm.rand(32, 40 * 512 + 100)
    a = d.file("a", data)
    b = d.clone("a", "b")
    edited, kept = (b, a) if edit_the == "clone" else (a, b)
    table, slots = d.p.fs.hashes(kept[0]).copy(), slots_of(c, d.p.fs, kept[0])
    # the same span count and size: the table is patched in place
    got = d.splice(edited, 7 * 512, 1024, dm.rand(33, 1024))
    assert got["spans_inserted"] == got["spans_removed"] == 3 and got["size_after"] == got["size_before"]
    assert (d.p.check_file(kept) == data).all()
    assert (d.p.fs.hashes(kept[0]) == table).all() and slots_of(c, d.p.fs, kept[0]) == slots
    # and one that builds a new table
    d.splice(edited, 100, 0, dm.rand(34, 77))
    d.splice(edited, 5000, 3000, None)
    assert (d.p.check_file(kept) == data).all()
    assert (d.p.fs.hashes(kept[0]) == table).all() and slots_of(c, d.p.fs, kept[0]) == slots
    r = d.diff(a, b)
    assert r["n_ranges"] >= 1 and r["size_a"] != r["size_b"]


def test_the_clone_outlives_the_original_through_a_collect():
    import chunkfs_amd as c
    d = Driver(c)
    p = d.p
    data = dm.rand(35, 64 << 10)
    d.file("a", data)
    d.clone("a", "b")
    p.open_files["a"], p.open_files["b"] = p.open("a"), p.open("b")
    p.remove("a")
    r = p.collect()
    assert r["containers_after"] == r["containers_before"] > 0 and r["bytes_moved"] == 0
    p.check_all()
    p.remove("b")
    r = p.collect()
    assert r["containers_after"] == 0 and r["arena_used_after"] == 0
    p.check_store()


def test_clone_of_an_empty_file_and_growth_past_the_clone_s_pool_class():
    import chunkfs_amd as c
    d = Driver(c)
    e = d.file("e", dm.rand(1, 0))
    e2 = d.clone("e", "e2")
    assert d.p.fs.stat(e2[0])["spans"] == 0 and d.diff(e, e2)["ranges"] == []
    d.p.append(e2, dm.rand(36, 100), [[0, 100]])  # and it takes spans like any file
    d.p.check_file(e2)
    assert d.p.fs.stat(e[0])["size"] == 0
    # 60 spans: a table of the 64-span class, whatever the source's capacity was
    data = dm.rand(37, 200 * 50)
    a = d.file("a", data, dm.tiling([50] * 200))  # capacity 256
    d.splice(a, 60 * 50, 140 * 50, None)  # 60 spans left
    b = d.clone("a", "b")
    more = dm.rand(38, 100 * 30)
    d.p.append(b, more, dm.tiling([30] * 100))  # past 64, then past 128
    assert (d.p.check_file(b) == np.concatenate([data[:3000], more])).all()
    assert (d.p.check_file(a) == data[:3000]).all()
    r = d.diff(a, b)
    assert r["ranges"] == [(3000, 3000)] and r["bytes_compared"] == 0


def test_clone_on_a_scrubbed_store_reads_equal():
    import chunkfs_amd as c
    fs = c.FileSystem.new_with_scrubber(c.CopyScrubber(), max_chunks=256, arena_bytes=MB,
                                        target_max_chunks=256, target_arena_bytes=MB)
    d = Driver(c, "fixed", fs=fs)
    data = dm.rand(39, 20 * 512 + 9)
    a = d.file("a", data)
    assert fs.scrub().processed_data == data.size
    b = d.clone("a", "b")
    assert (d.p.check_file(b, shift=1) == data).all() and (d.p.check_file(a) == data).all()
    # the diff, like collect and splice, refuses the scrubbed store and touches nothing
    st = c._lib.cdc_diff_stats_t(pieces=7)
    assert raw_diff(c, fs, a[0], b[0], stats=st) == c._lib.CDC_ENOTSUP and st.pieces == 7
    assert b"scrubbed" in c._lib.lib().cdc_last_error()


def test_clone_refusals_change_nothing():
    import chunkfs_amd as c
    d = Driver(c)
    data = dm.rand(40, 5000)
    d.file("a", data, dm.tiling([1000] * 5))
    d.file("other", data[:100], [[0, 100]])
    L, fs = c._lib.lib(), d.p.fs
    before, names = fs.store.stats(), fs.list_files()
    for args in ((None, b"a", b"x"), (fs._h, None, b"x"), (fs._h, b"a", None)):
        assert L.cdc_files_clone(*args, None) == c._lib.CDC_EINVAL
        assert b"NULL argument" in L.cdc_last_error()
    for src, dst, code in (("nope", "x", c._lib.CDC_ENOTFOUND), ("a", "other", c._lib.CDC_EEXIST),
                           ("a", "a", c._lib.CDC_EEXIST)):
        with pytest.raises(c.CdcError) as e:
            fs.clone_file(src, dst)
        assert _code(e) == code
    assert fs.store.stats() == before and fs.list_files() == names
    fs.store.clear()  # `a` is stale from here on
    with pytest.raises(c.CdcError) as e:
        fs.clone_file("a", "x")
    assert _code(e) == c._lib.CDC_ENOTFOUND and fs.list_files() == names


# ---- diff: the shared cases ------------------------------------------------------------------
def test_nothing_to_read():
    import chunkfs_amd as c
    d = Driver(c)
    dm.case_nothing_to_read(d)
    a, b = d.p.open("a", readonly=True), d.p.open("b", readonly=True)  # read-only handles are fine
    cursor = d.p.read_segment(a).size
    assert d.diff(a, b)["ranges"] == [] and d.p.fs.stat(a[0])["cursor"] == cursor > 0


@pytest.mark.parametrize("tables_only", [False, True])
@pytest.mark.parametrize("n", [1, 4096])
def test_one_edit(n, tables_only):
    import chunkfs_amd as c
    dm.case_one_edit(Driver(c), n, tables_only)


def test_run_and_piece_edges():
    import chunkfs_amd as c
    dm.case_edges(Driver(c))


def test_two_ranges_around_a_shared_span():
    import chunkfs_amd as c
    dm.case_two_ranges(Driver(c, "fixed"))


def test_the_tail():
    import chunkfs_amd as c
    dm.case_tail(Driver(c))


@pytest.mark.parametrize("L", dm.ALIGN_L)
def test_alignment_and_tiles(L):
    import chunkfs_amd as c
    dm.case_alignment(Driver(c), L)


@pytest.mark.parametrize("tables_only", [False, True])
def test_same_slot_shifted(tables_only):
    import chunkfs_amd as c
    dm.case_same_slot_shifted(Driver(c), tables_only)


def test_dense_and_long_masks():
    import chunkfs_amd as c
    dm.case_dense(Driver(c))


@pytest.mark.parametrize("n", list(dm.COUNT_CASES))
def test_counts_past_one_scan_block(n):
    import chunkfs_amd as c
    dm.case_counts(Driver(c, max_chunks=1 << 15), n)


@pytest.mark.parametrize("tables_only", [False, True])
def test_after_an_insert(tables_only):
    import chunkfs_amd as c
    for k in range(1, 18) if not tables_only else (1, 16, 17):
        dm.case_insert(Driver(c), k, tables_only)


# ---- cap -------------------------------------------------------------------------------------
def test_cap():
    import chunkfs_amd as c
    import torch
    d = Driver(c)
    data = dm.rand(41, 3000)
    a = d.file("a", data, dm.tiling([1000] * 3))
    b = d.file("b", dm.flipped(data, [5, 6, 1500, 2999]), dm.tiling([500] * 6))
    want = dm.diff(d.p.m, a[1], b[1])
    n = want["n_ranges"]
    assert n == 3
    for flags, exp in ((0, want), (c._lib.CDC_DIFF_TABLES_ONLY, dm.diff(d.p.m, a[1], b[1], True))):
        n = exp["n_ranges"]
        buf = torch.full((n + 2, 2), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")  # 0xA5 in every byte
        poison = buf.cpu().numpy().copy()
        torch.cuda.synchronize()
        st = c._lib.cdc_diff_stats_t()
        assert raw_diff(c, d.p.fs, a[0], b[0], flags, buf.data_ptr(), n - 1, st) == n
        assert (buf.cpu().numpy() == poison).all() and st.ranges == n  # nothing written, the stats filled
        assert st.bytes_differing == exp["bytes_differing"]
        assert raw_diff(c, d.p.fs, a[0], b[0], flags, None, 0, None) == n
        assert raw_diff(c, d.p.fs, a[0], b[0], flags, buf.data_ptr(), n, st) == n
        got = buf.cpu().numpy()
        assert [tuple(r) for r in got[:n].view(np.uint64).tolist()] == exp["ranges"]
        assert (got[n:] == poison[n:]).all()


def test_the_mirror_calls_again_when_its_buffer_is_too_small():
    import chunkfs_amd as c
    d = Driver(c)
    n = 4100  # 2050 ranges: more than the first buffer's 1024
    data = dm.rand(42, n)
    a = d.file("a", data, [[0, n]])
    b = d.file("b", dm.flipped(data, range(0, n, 2)), [[0, n]])
    assert d.diff(a, b)["n_ranges"] == 2050


# ---- refusals --------------------------------------------------------------------------------
def test_diff_refusals_touch_nothing():
    import chunkfs_amd as c
    import torch
    d = Driver(c)
    data = dm.rand(43, 2000)
    a = d.file("a", data, [[0, 2000]])
    b = d.file("b", data ^ 1, [[0, 2000]])
    other = Driver(c)
    x = other.file("x", data, [[0, 2000]])
    buf = torch.full((4, 2), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, E = c._lib.lib(), c._lib

    def refused(ha, hb, flags=0, ptr=buf.data_ptr(), cap=4):
        st = E.cdc_diff_stats_t(pieces=7, ranges=9)
        rc = L.cdc_files_diff_device(ha, hb, flags, ptr, cap, ctypes.byref(st), None)
        assert (st.pieces, st.ranges) == (7, 9) and (buf.cpu().numpy() == 7).all()
        return rc, L.cdc_last_error()

    assert refused(a[0]._fh, x[0]._fh) == (E.CDC_EINVAL, b"cdc_files_diff_device: the handles belong to two file layers")
    rc, msg = refused(a[0]._fh, b[0]._fh, flags=2)
    assert rc == E.CDC_EINVAL and b"unknown flag bits" in msg
    rc, msg = refused(a[0]._fh, b[0]._fh, flags=0x80000001)
    assert rc == E.CDC_EINVAL and b"unknown flag bits" in msg
    assert refused(a[0]._fh, None)[0] == E.CDC_EINVAL and refused(None, b[0]._fh)[0] == E.CDC_EINVAL
    rc, msg = refused(a[0]._fh, b[0]._fh, ptr=None)
    assert rc == E.CDC_EINVAL and b"NULL destination" in msg
    d.p.fs.remove_file("b")
    assert refused(a[0]._fh, b[0]._fh)[0] == E.CDC_ENOTFOUND and refused(b[0]._fh, a[0]._fh)[0] == E.CDC_ENOTFOUND
    b2 = d.p.fs.create_file("b", None)  # a new, empty file of that name: the old handle sees it
    assert raw_diff(c, d.p.fs, a[0], b[0]) == 1 and raw_diff(c, d.p.fs, a[0], b2) == 1
    d.p.fs.store.clear()  # a stale epoch
    assert refused(a[0]._fh, b2._fh)[0] == E.CDC_ENOTFOUND and refused(b2._fh, a[0]._fh)[0] == E.CDC_ENOTFOUND
    assert b"cleared" in L.cdc_last_error()


# ---- the C++ mirror ----------------------------------------------------------------------------
def test_cpp_snapshot_example_runs():
    import subprocess
    from chunkfs_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "_build", "files_snapshot_example")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(root, "include"), "-isystem", os.path.join(rocm, "include"),
                    os.path.join(root, "examples", "files_snapshot_example.cpp"),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd", "-L", os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
                    "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snapshot ok:" in r.stdout and "1 range {524365, 4096}" in r.stdout
