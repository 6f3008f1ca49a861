"""GPU suite of cdc_file_pack_device and cdc_files_unpack_device
(include/chunkfs_amd.h, "Packs: send and receive") against the model of
tests/pack_model.py.  Every pack is compared byte for byte with the model's and
every stats field but `seconds` with the model's; files are a few hundred KiB at
most, spans tens of bytes to a few KiB.  The shapes, the edits and the
corruptions are pack_model's, which tests/test_pack_model.py proves to keep the
contract and to be refused by the checks they are listed under."""
import ctypes
import os

import numpy as np
import pytest

import diff_model as dm
import pack_model as pm
import store_model as sm
from test_gpu_files import _code
from test_gpu_splice import SPair, slots_of

pytestmark = pytest.mark.gpu
MB = 1 << 20
SENTINEL = 0xA5


def stats(fs):
    """store.stats() without the ratios that are NaN on an empty store (NaN != NaN)."""
    return {k: v for k, v in fs.store.stats().items() if v == v}


def same(got, want):
    """PackStats against the model's dict, every field but seconds."""
    assert {k: getattr(got, k) for k in pm.STATS} == {k: want[k] for k in pm.STATS}, (got, want)
    assert got.seconds > 0


class Side(SPair):
    """One FileSystem with its model, packing and unpacking side by side."""

    def file(self, fname, data, chunks=None):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if chunks is None:
            return self.new_file(fname, data)
        hm = self.create(fname, self.chunker)
        if len(chunks):
            self.append(hm, data, chunks)
        return hm

    def clone(self, src, dst):
        assert self.fs.clone_file(src, dst) == dm.clone(self.m, src, dst)
        return self.open(dst, self.chunker)

    def pack(self, hm, since=None, have=None):
        """The pack as host bytes, compared with the model's; and the sizing call."""
        t, st = self.fs.pack(hm[0], since=since[0] if since else None, have=have)
        want, wst = pm.pack(self.m, hm[1], since=since[1] if since else None, have=have)
        blob = t.cpu().numpy().tobytes()
        assert len(blob) == len(want) and blob == want
        same(st, wst)
        if have is None:  # cap = 0 sizes the same pack
            assert self.fs.pack_device(hm[0], since[0] if since else None, None, None, 0) == len(want)
        return blob, st

    def unpack(self, name, blob, trust=False):
        want = pm.unpack(self.m, name, blob, trust=trust)
        got = self.fs.unpack(name, np.frombuffer(blob, dtype=np.uint8), hasher=None if trust else self.chunker,
                             trust=trust)
        same(got, want)
        self.seen.update(self.m.hashes(self.m.open(name)))
        return self.open(name, self.chunker)

    def state(self):
        return stats(self.fs), self.fs.list_files()


def twin_equal(a, ha, b, hb):
    """Two layers hold the same file in the same store: digests, span offsets,
    bytes, arena locations, and every field of stats().  (Which table slot a
    digest lands in is the parallel insert's to decide when two digests share a
    home slot, so slots are not compared.)"""
    assert stats(a.fs) == stats(b.fs)
    sm.assert_stats(b.fs.store, b.m.store)
    assert (a.fs.hashes(ha[0]) == b.fs.hashes(hb[0])).all()
    assert slots_of(a.c, a.fs, ha[0])[1] == slots_of(b.c, b.fs, hb[0])[1]
    assert (a.check_file(ha, shift=1) == b.check_file(hb, shift=2)).all()  # read_complete with its span offsets


# ---- the contract ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fast", "fixed"])
def test_full_pack_into_an_empty_store_equals_a_write(name):
    import chunkfs_amd as c
    data = pm.rand(51, 150 * 1024 + 13 if name == "fast" else 300 * 512 + 77)
    a, b, twin = Side(c, name), Side(c, name), Side(c, name)
    ha = a.file("f", data)
    blob, st = a.pack(ha)
    assert st.external_spans == 0 and st.chunks == st.spans > 100
    hb = b.unpack("f", blob)
    ht = twin.file("f", data)
    twin_equal(twin, ht, b, hb)
    twin_equal(a, ha, b, hb)
    assert (b.check_file(hb) == data).all()
    assert b.pack(hb)[0] == blob  # a fixed point
    b.check_reads("f")


SHAPES = pm.shapes()


@pytest.mark.parametrize("label", list(SHAPES))
def test_shapes(label):
    import chunkfs_amd as c
    data, chunks = SHAPES[label]
    big = len(chunks) > 1000
    kw = {"max_chunks": 1 << 13, "arena": 8 * MB}
    a, b, twin = Side(c, "fixed", **kw), Side(c, "fixed", **kw), Side(c, "fixed", **kw)
    ha = a.file("f", data, chunks)
    blob, st = a.pack(ha)
    if label == "empty":
        assert len(blob) == 64 and st.spans == 0
    if label == "heavy duplication":
        assert st.chunks == 2 and st.spans == 25
    if label == "padding lengths":
        assert st.chunk_bytes == 82 and st.pack_bytes - st.chunk_bytes > 46
    hb = b.unpack("f", blob, trust=big)  # the large ones also take the path without the hash
    ht = twin.file("f", data, chunks)
    twin_equal(twin, ht, b, hb)
    assert b.pack(hb)[0] == blob
    if not big and data.size:
        b.check_reads("f")


# ---- exclusions --------------------------------------------------------------------------------
def edited(c, name="fast"):
    """A sender with a base, its clone, and the file after one overwrite that
    patches the table in place and one insert that builds a new one."""
    a = Side(c, name)
    data = pm.rand(61, 96 << 10)
    h = a.file("a", data)
    base = a.clone("a", "base")
    got = a.splice(h, 78 * 512, 1024, pm.rand(62, 1024))
    assert got["size_after"] == got["size_before"]
    if name == "fixed":  # the same span count and size: the table is patched in place
        assert got["spans_inserted"] == got["spans_removed"]
    got = a.splice(h, 90000, 0, pm.rand(63, 300))  # and one that builds a new table
    assert got["size_after"] == got["size_before"] + 300
    return a, h, base


@pytest.mark.parametrize("name", ["fast", "fixed"])
def test_pack_against_a_clone_carries_the_new_chunks_only(name):
    import chunkfs_amd as c
    a, h, base = edited(c, name)
    b = Side(c, name)
    b.unpack("base", a.pack(base)[0])
    full, fst = a.pack(h)
    inc, st = a.pack(h, since=base)
    old = set(a.m.hashes(base[1]))
    new = {k for k in a.m.hashes(h[1]) if k not in old}
    assert st.chunks == len(new) > 0 and st.external_spans > 0 and len(inc) < len(full) // 4
    assert fst.chunks > 4 * st.chunks
    # `have` from the receiver's contains: the same pack, since it holds exactly the base
    dig = a.fs.hashes(h[0])
    dd = sm.dev(dig)
    import torch
    found = torch.zeros(len(dig), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b.fs.store.contains_device(dd.data_ptr(), len(dig), found.data_ptr())
    assert a.pack(h, have=found.cpu().numpy())[0] == inc
    assert a.fs.pack(h[0], have=found)[0].cpu().numpy().tobytes() == inc  # a device tensor as well
    before = b.fs.store.stats()
    hb = b.unpack("a", inc)
    after = b.fs.store.stats()
    assert after["unique_chunks"] - before["unique_chunks"] == st.chunks
    assert after["chunks_written"] - before["chunks_written"] == st.spans
    assert (b.check_file(hb) == a.check_file(h)).all()
    b.check_all()
    # since == fh carries nothing
    none, st0 = a.pack(h, since=h)
    assert st0.chunks == 0 and st0.external_spans == st0.spans and st0.chunk_bytes == 0
    b.unpack("a again", none)
    assert (b.check_file(b.open("a again")) == a.check_file(h)).all()


def test_unpack_without_the_base_is_refused_and_changes_nothing():
    import chunkfs_amd as c
    a, h, base = edited(c)
    inc, _ = a.pack(h, since=base)
    b = Side(c, "fast")
    b.file("other", pm.rand(64, 3000))
    before = b.state()
    with pytest.raises(c.CdcError) as e:
        b.fs.unpack("a", np.frombuffer(inc, np.uint8), hasher=b.chunker)
    assert _code(e) == c._lib.CDC_ENOTFOUND and "external span 0" in str(e.value)
    assert b.state() == before and not b.fs.file_exists("a")
    with pytest.raises(pm.PackError) as me:
        pm.unpack(b.m, "a", inc)
    assert me.value.code == pm.ENOTFOUND and me.value.index == 0


# ---- the Python paths ----------------------------------------------------------------------------
def test_send_between_two_file_systems_on_one_device():
    import chunkfs_amd as c
    a, h, base = edited(c)
    b = Side(c, "fast")
    sent, got = a.fs.send(base[0], b.fs, hasher=b.chunker)
    assert sent.chunks == got.chunks_new == sent.spans and got.external_spans == 0
    assert a.fs.store.stats()["unique_chunks"] > b.fs.store.stats()["unique_chunks"] == sent.chunks
    sent, got = a.fs.send(h[0], b.fs, name="a.v2")  # trusted: no hasher
    assert 0 < sent.chunks == got.chunks_new < 40 and got.external_spans == sent.external_spans > 0
    assert b.fs.list_files() == ["a.v2", "base"]
    hb = b.fs.open_file_readonly("a.v2")
    assert (b.fs.read_file_complete(hb) == a.check_file(h)).all()
    assert (b.fs.read_file_complete(b.fs.open_file_readonly("base")) == a.check_file(base)).all()
    st = b.fs.store.stats()
    assert st["chunks_written"] == a.fs.stat(h[0])["spans"] + a.fs.stat(base[0])["spans"]
    assert st["bytes_written"] == a.fs.stat(h[0])["size"] + a.fs.stat(base[0])["size"]
    sent, got = a.fs.send(h[0], b.fs, name="a.v3", hasher=b.chunker)  # everything is there already
    assert sent.chunks == 0 and got.chunks_new == 0 and sent.chunk_bytes == 0


def test_save_file_and_load_file(tmp_path):
    import chunkfs_amd as c
    a = Side(c, "fast")
    data = pm.rand(71, 70000)
    h = a.file("f", data)
    path = str(tmp_path / "f.pack")
    st = a.fs.save_file(h[0], path)
    assert os.path.getsize(path) == st.pack_bytes
    assert open(path, "rb").read() == pm.pack(a.m, h[1])[0]
    with pytest.raises(FileExistsError):
        a.fs.save_file(h[0], path)
    b = Side(c, "fast")
    got = b.fs.load_file("g", path, hasher=b.chunker)
    assert got.chunks_new == st.chunks and got.file_size == data.size
    assert (b.fs.read_file_complete(b.fs.open_file_readonly("g")) == data).all()
    assert stats(b.fs) == stats(a.fs)
    assert b.fs.load_file("g2", path, trust=True).chunks_new == 0


# ---- refusals change nothing -----------------------------------------------------------------------
def raw_pack(c, h, since=None, have=None, ptr=None, cap=0, stats=None):
    return c._lib.lib().cdc_file_pack_device(h._fh if h is not None else None,
                                             since._fh if since is not None else None, have, ptr, cap,
                                             ctypes.byref(stats) if stats is not None else None, None)


def raw_unpack(c, fs, name, t, length, hasher=None, flags=0, stats=None):
    return c._lib.lib().cdc_files_unpack_device(fs._h, name, ctypes.c_void_p(t.data_ptr()), length,
                                                hasher._h if hasher is not None else None, flags,
                                                ctypes.byref(stats) if stats is not None else None, None)


def test_cap_and_sizing():
    import chunkfs_amd as c
    import torch
    a = Side(c, "fixed")
    data, chunks = pm.corrupt_source()
    h = a.file("f", data, chunks)
    want, wst = pm.pack(a.m, h[1])
    need = len(want)
    buf = torch.full((need + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = a.state()
    st = c._lib.cdc_pack_stats_t()
    assert raw_pack(c, h[0], ptr=ctypes.c_void_p(buf.data_ptr()), cap=need - 1, stats=st) == need
    assert (buf.cpu().numpy() == SENTINEL).all()  # one byte short: the size, and nothing written
    assert (st.pack_bytes, st.chunks, st.spans) == (need, 4, 6)
    assert raw_pack(c, h[0], cap=0) == need  # cap = 0 sizes
    assert raw_pack(c, h[0], ptr=ctypes.c_void_p(buf.data_ptr()), cap=need) == need
    got = buf.cpu().numpy()
    assert got[:need].tobytes() == want and (got[need:] == SENTINEL).all()
    assert a.state() == before and a.fs.stat(h[0])["cursor"] == 0
    ro = a.fs.open_file_readonly("f")  # read-only handles are fine
    assert a.fs.pack(ro)[0].cpu().numpy().tobytes() == want


def test_pack_refusals():
    import chunkfs_amd as c
    import torch
    E, L = c._lib, c._lib.lib()
    a, other = Side(c, "fixed"), Side(c, "fixed")
    data = pm.rand(81, 3000)
    h = a.file("f", data)
    g = a.file("g", data[:1000])
    x = other.file("x", data)
    buf = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = ctypes.c_void_p(buf.data_ptr())

    def refused(hh, since=None, p=ptr, cap=1 << 16):
        st = E.cdc_pack_stats_t(chunks=7, spans=9)
        before = a.state()
        rc = raw_pack(c, hh, since, None, p, cap, st)
        msg = L.cdc_last_error()
        assert (st.chunks, st.spans) == (7, 9) and (buf.cpu().numpy() == SENTINEL).all() and a.state() == before
        return rc, msg

    rc, msg = refused(h[0], since=x[0])
    assert rc == E.CDC_EINVAL and b"another file layer" in msg
    rc, msg = refused(h[0], p=ctypes.c_void_p(buf.data_ptr() + 8))
    assert rc == E.CDC_EINVAL and b"not 16-byte aligned" in msg
    rc, msg = refused(h[0], p=None)
    assert rc == E.CDC_EINVAL and b"NULL destination" in msg
    assert refused(None)[0] == E.CDC_EINVAL
    a.fs.remove_file("g")
    assert refused(g[0])[0] == E.CDC_ENOTFOUND and refused(h[0], since=g[0])[0] == E.CDC_ENOTFOUND
    a.fs.clear_database()  # the handle's file is gone with everything else
    assert refused(h[0])[0] == E.CDC_ENOTFOUND
    # a handle that outlives a store clear is stale
    b = Side(c, "fixed")
    hb = b.file("f", data)
    keep = b.file("k", data[:512])
    b.fs.store.clear()
    st = E.cdc_pack_stats_t(chunks=7)
    assert raw_pack(c, hb[0], None, None, ptr, 1 << 16, st) == E.CDC_ENOTFOUND and b"cleared" in L.cdc_last_error()
    assert raw_pack(c, keep[0], hb[0], None, ptr, 1 << 16, st) == E.CDC_ENOTFOUND and st.chunks == 7
    assert (buf.cpu().numpy() == SENTINEL).all()


def test_unpack_refusals_change_nothing():
    import chunkfs_amd as c
    E = c._lib
    a = Side(c, "fixed")
    data, chunks = pm.corrupt_source()
    h = a.file("f", data, chunks)
    blob, st = a.pack(h)
    arr = np.frombuffer(blob, np.uint8)
    # the name exists
    b = Side(c, "fixed")
    b.unpack("f", blob)
    before = b.state()
    with pytest.raises(c.CdcError) as e:
        b.fs.unpack("f", arr, hasher=b.chunker)
    assert _code(e) == E.CDC_EEXIST and b.state() == before
    # an arena one padded chunk too small, a table one chunk too small: as if every chunk were new
    arena = sum(pm.pad16(ln) for ln in (100, 32, 17, 1))
    for kw, mkw in (({"max_chunks": 16, "arena_bytes": arena - 16}, {"arena": arena - 16}),
                    ({"max_chunks": st.chunks - 1, "arena_bytes": MB}, {"max_chunks": st.chunks - 1})):
        fs = c.FileSystem(**kw)
        before = (stats(fs), fs.list_files())
        with pytest.raises(c.CdcError) as e:
            fs.unpack("f", arr, trust=True)
        assert _code(e) == E.CDC_ENOMEM and (stats(fs), fs.list_files()) == before
        with pytest.raises(pm.PackError) as me:
            pm.unpack(b.m.__class__(), "f", blob, **mkw)
        assert me.value.code == pm.ENOMEM
    fs = c.FileSystem(max_chunks=st.chunks, arena_bytes=arena)
    assert fs.unpack("f", arr, trust=True).chunks_new == st.chunks  # exactly enough
    assert fs.store.stats()["arena_used"] == arena
    # a hasher is needed unless the pack is trusted
    with pytest.raises(c.CdcError) as e:
        c.FileSystem(max_chunks=16, arena_bytes=MB).unpack("f", arr)
    assert _code(e) == E.CDC_EINVAL and "NULL hasher" in str(e.value)


def test_a_scrubbed_store_is_not_supported_in_either_direction():
    import chunkfs_amd as c
    import torch
    E, L = c._lib, c._lib.lib()
    fs = c.FileSystem.new_with_scrubber(c.CopyScrubber(), max_chunks=256, arena_bytes=MB,
                                        target_max_chunks=256, target_arena_bytes=MB)
    a = Side(c, "fixed", fs=fs)
    data = pm.rand(91, 10 * 512 + 9)
    h = a.file("f", data)
    good = a.fs.pack(h[0])[0]
    assert fs.scrub().processed_data == data.size
    st = E.cdc_pack_stats_t(chunks=7)
    before = (stats(fs), fs.list_files())
    assert raw_pack(c, h[0], cap=0, stats=st) == E.CDC_ENOTSUP and b"scrubbed" in L.cdc_last_error()
    torch.cuda.synchronize()
    assert raw_unpack(c, fs, b"g", good, good.numel(), flags=1, stats=st) == E.CDC_ENOTSUP
    assert b"scrubbed" in L.cdc_last_error() and st.chunks == 7
    assert (stats(fs), fs.list_files()) == before


# ---- corrupt packs: refused by the named check, nothing changed ----------------------------------------
def corrupt_cases():
    data, chunks = pm.corrupt_source()
    files = pm.fm.Files()
    h = files.create("f")
    files.append(h, data, chunks)
    good, _ = pm.pack(files, h)
    return good, pm.corruptions(good)


GOOD, CORRUPT = corrupt_cases()


def test_the_device_pack_is_the_one_the_corruptions_edit():
    import chunkfs_amd as c
    a = Side(c, "fixed")
    h = a.file("f", *pm.corrupt_source())
    assert a.pack(h)[0] == GOOD


@pytest.mark.parametrize("case", CORRUPT, ids=[x[0] for x in CORRUPT])
def test_corrupt_packs(case):
    import chunkfs_amd as c
    import torch
    label, blob, length, trust, code, check = case
    E, L = c._lib, c._lib.lib()
    b = Side(c, "fixed", max_chunks=64, arena=MB)
    b.file("other", pm.rand(95, 700))
    before = b.state()
    t = sm.dev(np.frombuffer(blob, np.uint8).copy())
    st = E.cdc_pack_stats_t(chunks=7, spans=9)
    rc = raw_unpack(c, b.fs, b"f", t, length, None if trust else b.chunker, 1 if trust else 0, st)
    msg = L.cdc_last_error().decode()
    if code == 0:  # what CDC_UNPACK_TRUST means: the flipped byte is stored and read back
        assert rc == 6 and st.chunks_new == 4
        data, _ = pm.corrupt_source()
        back = b.fs.read_file_complete(b.fs.open_file_readonly("f"))
        assert np.nonzero(back != data)[0].tolist() == [100, 249]
        return
    assert rc == code, (label, rc, msg)
    want = {"hash": "does not hash to its digest", "len < 64": "len < 64"}.get(check, "pack check '%s'" % check)
    assert want in msg, (label, msg)
    with pytest.raises(pm.PackError) as me:
        pm.unpack(pm.fm.Files(), "f", blob, trust=trust, length=length)
    if check not in ("len < 64",):
        assert ("index %d " % me.value.index) in msg or ("chunk %d " % me.value.index) in msg, (label, msg)
    assert (st.chunks, st.spans) == (7, 9) and b.state() == before and not b.fs.file_exists("f")
    torch.cuda.synchronize()
    b.check_all()  # and the layer goes on working


# ---- the C++ mirror ------------------------------------------------------------------------------
def test_cpp_pack_example_runs():
    import subprocess
    from chunkfs_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "_build", "files_pack_example")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(root, "include"), "-isystem", os.path.join(rocm, "include"),
                    os.path.join(root, "examples", "files_pack_example.cpp"),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd", "-L", os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
                    "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pack ok:" in r.stdout
