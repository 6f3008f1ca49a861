"""GPU suite of cdc_files_delta_device (include/chunkfs_amd.h, "Content-aligned
delta") against the model of tests/delta_model.py.  After every delta the ops
and every stats field but `seconds` equal the model's, and apply_delta of the
ops and their literals gives read_file_complete of B.  The cases are
delta_model's, which tests/test_delta_model.py runs on the model alone; files
are a few hundred KiB at most, spans tens of bytes to a few KiB."""
import ctypes
import os

import numpy as np
import pytest

import delta_model as dl
from test_gpu_snapshot import Driver as SnapshotDriver

pytestmark = pytest.mark.gpu
MB = 1 << 20
LIT = dl.LIT


class Driver(SnapshotDriver):
    """delta_model's cases on the device layer, the model beside it."""

    def delta(self, a, b, tables_only=False):
        fs = self.p.fs
        got = fs.delta(a[0], b[0], tables_only=tables_only, literals=True)
        want = dl.delta(self.p.m, a[1], b[1], tables_only)
        assert got.ops.dtype == np.uint64 and got.ops.shape == (got.n_ops, 3)
        ops = [tuple(r) for r in got.ops.tolist()]
        assert ops == want["ops"], (ops[:8], want["ops"][:8])
        for k in dl.STATS:
            assert getattr(got, k) == want[k], (k, getattr(got, k), want[k])
        assert got.seconds > 0 and got.literals.numel() == want["bytes_literal"]
        rebuilt = fs.apply_delta(a[0], got.ops, got.literals).cpu().numpy()
        assert (rebuilt == fs.read_file_complete(b[0])).all() and rebuilt.size == want["size_b"]
        return dict({k: getattr(got, k) for k in dl.STATS}, ops=ops)


def raw_delta(c, a, b, flags=0, d_ops=None, cap=0, stats=None):
    return c._lib.lib().cdc_files_delta_device(a._fh, b._fh, flags, d_ops, cap,
                                               ctypes.byref(stats) if stats is not None else None, None)


# ---- the shared cases ------------------------------------------------------------------------
def test_the_prototype_table():
    import chunkfs_amd as c
    dl.case_prototype(Driver(c, "fixed"))


@pytest.mark.parametrize("name", ["fixed", "fast"])
def test_insert_at_offset_0(name):
    """diff_model.case_insert's scenario: one LITERAL of k bytes, one COPY of the rest."""
    import chunkfs_amd as c
    for k in range(1, 18):
        dl.case_insert(Driver(c, name), k)
    dl.case_insert(Driver(c, name), 5, True)


@pytest.mark.parametrize("tables_only", [False, True])
def test_edits_in_the_middle(tables_only):
    import chunkfs_amd as c
    dl.case_edits(Driver(c), tables_only)


@pytest.mark.parametrize("L", dl.ALIGN_L)
def test_alignment_and_tiles(L):
    import chunkfs_amd as c
    dl.case_alignment(Driver(c), L)
    dl.case_misalign(Driver(c), L)


def test_forward_and_backward_overlap():
    import chunkfs_amd as c
    dl.case_overlap(Driver(c))


def test_the_nearest_rule():
    import chunkfs_amd as c
    dl.case_nearest(Driver(c, max_chunks=1 << 14))


def test_spans_of_length_0():
    import chunkfs_amd as c
    dl.case_empty_spans(Driver(c))


def test_degenerate_sizes_and_contents():
    import chunkfs_amd as c
    d = Driver(c)
    dl.case_degenerate(d)
    a, e = d.p.open("a", readonly=True), d.p.open("e1", readonly=True)  # read-only handles are fine
    cursor = d.p.read_segment(a).size
    assert d.delta(a, a)["ops"] == [(0, 3000, 0)] and d.delta(e, a)["ops"] == [(0, 3000, LIT)]
    assert d.p.fs.stat(a[0])["cursor"] == cursor > 0


@pytest.mark.parametrize("changed,lead", list(dl.COUNT_CASES))
def test_counts_past_one_scan_block(changed, lead):
    import chunkfs_amd as c
    dl.case_counts(Driver(c, max_chunks=1 << 15), changed, lead)


def test_a_blake2sp_layer():
    import chunkfs_amd as c
    fs = c.FileSystem(max_chunks=1 << 12, arena_bytes=8 * MB, hash="blake2sp")
    ch = c.FastChunker(c.SizeParams(64, 256, 1024))
    data = dl.rand(95, 64 << 10)
    a = fs.create_file("a", ch)
    fs.write_to_file(a, data)
    fs.clone_file("a", "b")
    b = fs.open_file("b", ch)
    fs.splice(b, 30000, 0, dl.rand(96, 9))
    r = fs.delta(a, b, literals=True)
    assert [tuple(x) for x in r.ops.tolist()] == [(0, 30000, 0), (30000, 9, LIT), (30009, data.size - 30000, 30000)]
    assert r.spans_matched > 0 and r.regions == 1 and 9 <= r.bytes_literal_tables < 4096
    assert (fs.apply_delta(a, r.ops, r.literals).cpu().numpy() == fs.read_file_complete(b)).all()


# ---- cap -------------------------------------------------------------------------------------
def test_cap():
    import chunkfs_amd as c
    import torch
    d = Driver(c)
    data = dl.rand(41, 3000)
    a = d.file("a", data, dl.tiling([1000] * 3))
    b = d.file("b", dl.flipped(data, [5, 6, 1500]), dl.tiling([500] * 6))
    e = d.file("e", data[:0])
    for ha, flags in ((a, 0), (a, c._lib.CDC_DELTA_TABLES_ONLY), (e, 0)):
        exp = dl.delta(d.p.m, ha[1], b[1], bool(flags))
        n = exp["n_ops"]
        assert n == (1 if ha is e or flags else 3)
        buf = torch.full((n + 2, 3), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")  # 0xA5 in every byte
        poison = buf.cpu().numpy().copy()
        torch.cuda.synchronize()
        st = c._lib.cdc_delta_stats_t()
        assert raw_delta(c, ha[0], b[0], flags, buf.data_ptr(), n - 1, st) == n
        assert (buf.cpu().numpy() == poison).all() and st.ops == n  # nothing written, the stats filled
        assert (st.bytes_literal, st.bytes_copy) == (exp["bytes_literal"], exp["bytes_copy"])
        assert raw_delta(c, ha[0], b[0], flags, None, 0, None) == n
        assert raw_delta(c, ha[0], b[0], flags, buf.data_ptr(), n, st) == n
        got = buf.cpu().numpy()
        assert [tuple(r) for r in got[:n].view(np.uint64).tolist()] == exp["ops"]
        assert (got[n:] == poison[n:]).all()
        buf.copy_(torch.from_numpy(poison))
        assert raw_delta(c, ha[0], b[0], flags, buf.data_ptr(), n + 2, st) == n
        got = buf.cpu().numpy()
        assert [tuple(r) for r in got[:n].view(np.uint64).tolist()] == exp["ops"] and (got[n:] == poison[n:]).all()


def test_the_mirror_calls_again_when_its_buffer_is_too_small():
    import chunkfs_amd as c
    d = Driver(c, max_chunks=1 << 15)
    assert dl.case_counts(d, 1024, True)["exact"]["n_ops"] == 2049  # more than the first buffer's 1024


# ---- refusals --------------------------------------------------------------------------------
def test_delta_refusals_touch_nothing():
    import chunkfs_amd as c
    import torch
    d = Driver(c)
    data = dl.rand(43, 2000)
    a = d.file("a", data, [[0, 2000]])
    b = d.file("b", data ^ 1, [[0, 2000]])
    other = Driver(c)
    x = other.file("x", data, [[0, 2000]])
    buf = torch.full((4, 3), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, E = c._lib.lib(), c._lib

    def refused(ha, hb, flags=0, ptr=buf.data_ptr(), cap=4):
        st = E.cdc_delta_stats_t(regions=7, ops=9)
        rc = L.cdc_files_delta_device(ha, hb, flags, ptr, cap, ctypes.byref(st), None)
        assert (st.regions, st.ops) == (7, 9) and (buf.cpu().numpy() == 7).all()
        return rc, L.cdc_last_error()

    assert refused(a[0]._fh, x[0]._fh) == (E.CDC_EINVAL,
                                           b"cdc_files_delta_device: the handles belong to two file layers")
    for flags in (2, 0x80000001):
        rc, msg = refused(a[0]._fh, b[0]._fh, flags=flags)
        assert rc == E.CDC_EINVAL and b"unknown flag bits" in msg
    assert refused(a[0]._fh, None)[0] == E.CDC_EINVAL and refused(None, b[0]._fh)[0] == E.CDC_EINVAL
    rc, msg = refused(a[0]._fh, b[0]._fh, ptr=None)
    assert rc == E.CDC_EINVAL and b"NULL destination" in msg
    d.p.fs.remove_file("b")
    assert refused(a[0]._fh, b[0]._fh)[0] == E.CDC_ENOTFOUND and refused(b[0]._fh, a[0]._fh)[0] == E.CDC_ENOTFOUND
    b2 = d.p.fs.create_file("b", None)  # a new, empty file of that name: the old handle sees it
    assert raw_delta(c, a[0], b[0]) == 0 and raw_delta(c, b2, a[0]) == 1
    d.p.fs.store.clear()  # a stale epoch
    assert refused(a[0]._fh, b2._fh)[0] == E.CDC_ENOTFOUND and refused(b2._fh, a[0]._fh)[0] == E.CDC_ENOTFOUND
    assert b"cleared" in L.cdc_last_error()


def test_delta_refuses_a_scrubbed_store():
    import chunkfs_amd as c
    fs = c.FileSystem.new_with_scrubber(c.CopyScrubber(), max_chunks=256, arena_bytes=MB,
                                        target_max_chunks=256, target_arena_bytes=MB)
    d = Driver(c, "fixed", fs=fs)
    data = dl.rand(39, 20 * 512 + 9)
    a = d.file("a", data)
    assert fs.scrub().processed_data == data.size
    b = d.clone("a", "b")
    st = c._lib.cdc_delta_stats_t(regions=7)
    assert raw_delta(c, a[0], b[0], stats=st) == c._lib.CDC_ENOTSUP and st.regions == 7
    assert b"scrubbed" in c._lib.lib().cdc_last_error()


# ---- the C++ mirror ----------------------------------------------------------------------------
def test_cpp_delta_example_runs():
    import subprocess
    from chunkfs_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "_build", "files_delta_example")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(root, "include"), "-isystem", os.path.join(rocm, "include"),
                    os.path.join(root, "examples", "files_delta_example.cpp"),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd", "-L", os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
                    "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "delta ok: 3 ops" in r.stdout
    assert "COPY {0, 524365, 0}" in r.stdout and "LITERAL {524365, 4096}" in r.stdout
    assert "COPY {528461, 524211, 524365}" in r.stdout
