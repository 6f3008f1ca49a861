"""Device chunk store (include/chunkfs_amd.h "Chunk store") against the
reference semantics: Database insert / get_multi / contains with the first
insert winning (src/system/database.rs:10-36, 74-87), ChunkStorage::retrieve
(src/system/storage.rs:141-157) and read_file_complete (src/system/mod.rs:
149-160).  The oracle is store_model.Model, a dict fed in chunk order; every
comparison of bytes is exact.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import store_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWEEP_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 12289]


def _code(excinfo):
    return excinfo.value.code


def test_alignment_and_length_sweep():
    """Every source offset mod 16 x every length class through put; every length
    class at every destination offset mod 16 through get."""
    import chunkfs_amd as c
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, 256 << 10, dtype=np.uint8)
    chunks = []
    for ci, ln in enumerate(SWEEP_LENGTHS):
        for m in range(16):
            chunks.append((16 * 37 * len(chunks) + m, ln))  # distinct offsets, source offset mod 16 = m
    chunks = np.array(chunks, dtype=np.uint64)
    assert int((chunks[:, 0] + chunks[:, 1]).max()) <= data.size
    assert {(int(o) % 16, int(ln)) for o, ln in chunks} == {(m, ln) for m in range(16) for ln in SWEEP_LENGTHS}
    model = sm.Model()
    dig, want_new = model.put(data, chunks)
    d_data = sm.dev(data)
    st = c.ChunkStore(1024, 1 << 20)
    new = sm.put(st, d_data, data.size, chunks, dig)
    assert (new == want_new).all()
    sm.assert_stats(st, model)
    assert st.stats()["arena_used"] == sum(sm.round_up16(len(b)) for b in model.db.values())

    sm.get_checked(st, model, dig[::-1])
    # Every length class on every destination offset mod 16: 1-byte chunks pad
    # the running offset up to the wanted residue before each chunk.
    one = dig[SWEEP_LENGTHS.index(1) * 16]
    order, at = [], 0
    for t in range(16):
        for ci, ln in enumerate(SWEEP_LENGTHS):
            while at % 16 != t:
                order.append(one)
                at += 1
            order.append(dig[ci * 16 + (t * 7 + ci) % 16])
            at += ln
    order = np.array(order, dtype=np.uint8)
    spans = sm.get_checked(st, model, order)
    seen = {(int(o) % 16, int(ln)) for o, ln in spans}
    assert seen >= {(t, ln) for t in range(16) for ln in SWEEP_LENGTHS}, "the request order missed a pair"
    sm.get_checked(st, model, order[: len(order) // 3], shift=5)  # d_out itself off the 16-byte grid


def _versions():
    """A base blob plus three mutated copies (the construction of the index test)."""
    rng = np.random.default_rng(3)
    versions = [oracle.splitmix64_bytes(2 << 20, 7)]
    for k in range(3):
        v = versions[-1].copy()
        for _ in range(20):  # overwrite / insert / delete small runs
            p = int(rng.integers(0, v.size - 5000))
            if k % 3 == 0:
                v[p:p + 100] = rng.integers(0, 256, 100, dtype=np.uint8)
            elif k % 3 == 1:
                v = np.concatenate([v[:p], rng.integers(0, 256, 333, dtype=np.uint8), v[p:]])
            else:
                v = np.concatenate([v[:p], v[p + 777:]])
        versions.append(v)
    return versions


def test_versioned_data_round_trip():
    import chunkfs_amd as c
    ch = c.FastChunker(c.SizeParams(4096, 8192, 16384))
    st = c.ChunkStore(1 << 13, 12 << 20)
    model, files = sm.Model(), []
    for v in _versions():
        chunks, dig = ch.chunk_and_hash(v)
        want_dig, want_new = model.put(v, chunks)
        assert (dig == want_dig).all()
        new = sm.put(st, sm.dev(v), v.size, chunks, dig)
        assert (new == want_new).all()
        sm.assert_stats(st, model)
        files.append((v, dig))
    for v, dig in files:
        want, _ = model.read(dig)
        assert (want == v).all()
        sm.get_checked(st, model, dig)
        assert (st.read(dig) == v).all()
    assert st.stats()["cdc_dedup_ratio"] > 1.5  # the copies share most chunks


def test_write_and_read_conveniences():
    import chunkfs_amd as c
    ch = c.FastChunker(c.SizeParams(4096, 8192, 16384))
    st = c.ChunkStore(1 << 10, 3 << 20)  # room for the second write as if it were all new
    data = oracle.splitmix64_bytes((1 << 20) + 13, 21)
    chunks, dig, new = st.write(ch, data)
    assert new.all() and int(chunks[:, 1].sum()) == data.size
    _, _, again = st.write(ch, data)
    assert not again.any()
    assert (st.read(dig) == data).all()
    assert st.read(np.zeros((0, 32), dtype=np.uint8)).size == 0


def test_batch_form_equals_single_form():
    import torch
    import chunkfs_amd as c
    a = oracle.splitmix64_bytes((1 << 20) + 77, 31)
    b = oracle.splitmix64_bytes(300001, 32)
    shared = np.concatenate([a[:400000], oracle.splitmix64_bytes(200003, 33)])  # shares a prefix with a
    hosts = [a, np.zeros(0, dtype=np.uint8), b, a.copy(), shared]
    lens = [h.size for h in hosts]
    bufs = [sm.dev(h if h.size else np.zeros(1, dtype=np.uint8)) for h in hosts]
    ptrs = [t.data_ptr() for t in bufs]
    ch = c.FastChunker(c.SizeParams(4096, 8192, 16384))
    cap = ch.batch_max_chunks(lens)
    out = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    first = ch.chunk_batch_device(ptrs, lens, out.data_ptr(), cap)
    n = int(first[-1])
    dig = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    ch.sha256_batch_device(ptrs, first, out.data_ptr(), dig.data_ptr())
    h_chunks, h_dig = out[:n].cpu().numpy().view(np.uint64), dig.cpu().numpy()

    model = sm.Model()
    want_new = []
    for i, h in enumerate(hosts):
        z0, z1 = int(first[i]), int(first[i + 1])
        d, f = model.put(h, h_chunks[z0:z1])
        assert (d == h_dig[z0:z1]).all()
        want_new.append(f)
    want_new = np.concatenate(want_new)

    sa, sb = c.ChunkStore(1 << 12, 8 << 20), c.ChunkStore(1 << 12, 8 << 20)
    new_a = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n_new = sa.put_batch_device(ptrs, lens, first, out.data_ptr(), dig.data_ptr(), new_a.data_ptr())
    new_a = new_a.cpu().numpy().astype(bool)
    assert n_new == int(new_a.sum())
    new_b = np.concatenate([sm.put(sb, bufs[i], lens[i], h_chunks[int(first[i]):int(first[i + 1])],
                                   h_dig[int(first[i]):int(first[i + 1])]) for i in range(len(hosts))])
    assert (new_a == want_new).all() and (new_b == want_new).all()
    assert sa.stats() == sb.stats()
    sm.assert_stats(sa, model)
    assert not want_new[int(first[3]):int(first[4])].any()  # the copy adds nothing
    for i, h in enumerate(hosts):
        d = h_dig[int(first[i]):int(first[i + 1])]
        if len(d):
            sm.get_checked(sa, model, d)
            sm.get_checked(sb, model, d)
            assert (sa.read(d) == h).all()


def test_many_tiny_chunks():
    """20 000 chunks of 1..7 bytes: heavy in-batch duplication, scans over many blocks."""
    import chunkfs_amd as c
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 64 << 10, dtype=np.uint8)
    n = 20000
    lens = rng.integers(1, 8, n).astype(np.uint64)
    offs = rng.integers(0, data.size - 8, n).astype(np.uint64)
    chunks = np.stack([offs, lens], axis=1)
    model = sm.Model()
    dig, want_new = model.put(data, chunks)
    assert 0 < int(want_new.sum()) < n
    st = c.ChunkStore(n, n * 16)
    new = sm.put(st, sm.dev(data), data.size, chunks, dig)
    assert (new == want_new).all()
    sm.assert_stats(st, model)
    sm.get_checked(st, model, dig)


def test_one_large_chunk():
    """3 MiB + 5 at source offset 7, read back behind a 3-byte chunk (misaligned destination)."""
    import chunkfs_amd as c
    big = (3 << 20) + 5
    data = oracle.splitmix64_bytes(7 + big + 9, 77)
    chunks = np.array([[1, 3], [7, big]], dtype=np.uint64)
    model = sm.Model()
    dig, want_new = model.put(data, chunks)
    st = c.ChunkStore(16, 4 << 20)
    new = sm.put(st, sm.dev(data), data.size, chunks, dig)
    assert (new == want_new).all() and new.all()
    sm.assert_stats(st, model)
    spans = sm.get_checked(st, model, dig)
    assert spans.tolist() == [[0, 3], [3, big]]


def _small_store(c, seed=1, n=40, length=100, **kw):
    """A store holding n chunks of `length` bytes of one random buffer."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, n * length, dtype=np.uint8)
    chunks = np.array([[i * length, length] for i in range(n)], dtype=np.uint64)
    model = sm.Model()
    dig, _ = model.put(data, chunks)
    st = c.ChunkStore(kw.get("max_chunks", 256), kw.get("arena_bytes", 1 << 16))
    assert sm.put(st, sm.dev(data), data.size, chunks, dig).all()
    return st, model, dig


def test_not_found():
    import torch
    import chunkfs_amd as c
    st, model, dig = _small_store(c)
    before = st.stats()
    req = dig[:9].copy()
    req[4] = np.frombuffer(bytes(range(32)), dtype=np.uint8)  # absent
    dd = sm.dev(req)
    g = sm.Guarded(900, 9)
    with pytest.raises(c.CdcError) as ei:
        st.get_device(dd.data_ptr(), 9, g.out_ptr, 900, g.spans.data_ptr())
    assert _code(ei) == c._lib.CDC_ENOTFOUND
    g.assert_untouched()
    assert st.stats() == before
    found = torch.full((9,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert st.contains_device(dd.data_ptr(), 9, found.data_ptr()) == 8
    assert found.cpu().numpy().tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]
    assert st.stats() == before
    sm.get_checked(st, model, dig)


def test_lookup_probes_past_64_bit_key_collisions():
    """Digests are the caller's: four that share the index's 64-bit key (first 8
    bytes, bit 0 ignored) but differ later must each give their own chunk back,
    and a fifth with the same key that was never stored must be absent."""
    import torch
    import chunkfs_amd as c
    rng = np.random.default_rng(13)
    data = rng.integers(0, 256, 4096, dtype=np.uint8)
    chunks = np.array([[0, 100], [100, 33], [133, 1000], [1133, 7], [2000, 50]], dtype=np.uint64)
    dig = np.zeros((6, 32), dtype=np.uint8)
    dig[:, :8] = np.frombuffer(bytes([0x10, 2, 3, 4, 5, 6, 7, 8]), dtype=np.uint8)
    dig[1, 0] = 0x11          # same key once bit 0 is forced
    dig[2, 8] = 1             # differs in the second 8 bytes
    dig[3, 31] = 1            # differs in the last byte
    dig[4] = rng.integers(0, 256, 32, dtype=np.uint8)  # an unrelated digest
    dig[5, 16] = 9            # same key, never stored
    model = sm.Model()
    for d, (o, ln) in zip(dig[:5], chunks):
        model.db[bytes(d)] = data[int(o):int(o) + int(ln)].tobytes()
    model.chunks_written, model.bytes_written = 5, int(chunks[:, 1].sum())
    st = c.ChunkStore(64, 1 << 14)
    assert sm.put(st, sm.dev(data), data.size, chunks, dig[:5]).all()
    sm.assert_stats(st, model)
    sm.get_checked(st, model, dig[[3, 0, 4, 2, 1, 0]])
    again = sm.put(st, sm.dev(data), data.size, chunks[::-1].copy(), dig[:5])  # other bytes, known digests
    assert not again.any()
    sm.get_checked(st, model, dig[:5])  # the first insert's bytes
    dd = sm.dev(dig)
    found = torch.zeros(6, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert st.contains_device(dd.data_ptr(), 6, found.data_ptr()) == 5
    assert found.cpu().numpy().tolist() == [1, 1, 1, 1, 1, 0]
    with pytest.raises(c.CdcError) as ei:
        st.get_device(dd.data_ptr(), 6, None, 0)
    assert _code(ei) == c._lib.CDC_ENOTFOUND


def test_sizing_and_refusal():
    import chunkfs_amd as c
    # sizing: out_cap = 0 and out_cap = total - 1 write nothing
    st, model, dig = _small_store(c)
    dd = sm.dev(dig)
    total = 40 * 100
    assert st.get_device(dd.data_ptr(), 40, None, 0) == total
    g = sm.Guarded(total, 40)
    assert st.get_device(dd.data_ptr(), 40, g.out_ptr, 0, g.spans.data_ptr()) == total
    assert st.get_device(dd.data_ptr(), 40, g.out_ptr, total - 1, g.spans.data_ptr()) == total
    g.assert_untouched()

    rng = np.random.default_rng(9)
    more = rng.integers(0, 256, 4000, dtype=np.uint8)
    more_chunks = np.array([[i * 100, 100] for i in range(40)], dtype=np.uint64)
    more_dig, _ = sm.Model().put(more, more_chunks)
    d_more = sm.dev(more)
    # arena: 40 chunks of 100 bytes take 40 * 112; room for the first batch, not for a second all-new one
    st, model, dig = _small_store(c, arena_bytes=40 * 112 + 39 * 112 + 111)
    before = st.stats()
    with pytest.raises(c.CdcError) as ei:
        sm.put(st, d_more, more.size, more_chunks, more_dig)
    assert _code(ei) == c._lib.CDC_ENOMEM
    assert st.stats() == before
    sm.get_checked(st, model, dig)
    # conservative: a batch of known chunks is refused too, as if every chunk were new
    with pytest.raises(c.CdcError) as ei:
        sm.put(st, d_more, more.size, more_chunks[:1].repeat(40, axis=0), more_dig[:1].repeat(40, axis=0))
    assert _code(ei) == c._lib.CDC_ENOMEM
    assert st.stats() == before
    # ... and one that fits exactly is taken
    assert sm.put(st, d_more, more.size, more_chunks[:39], more_dig[:39]).all()

    # max_chunks
    st, model, dig = _small_store(c, max_chunks=79)
    before = st.stats()
    with pytest.raises(c.CdcError) as ei:
        sm.put(st, d_more, more.size, more_chunks, more_dig)
    assert _code(ei) == c._lib.CDC_ENOMEM
    assert st.stats() == before
    sm.get_checked(st, model, dig)

    # a chunk that leaves its buffer, single and batch form
    st, model, dig = _small_store(c)
    before = st.stats()
    for bad in ([3901, 100], [4001, 0], [0, 4001], [2 ** 64 - 50, 100], [100, 2 ** 64 - 50], [0, 2 ** 64 - 1]):
        bad_chunks = more_chunks.copy()
        bad_chunks[17] = bad
        with pytest.raises(c.CdcError) as ei:
            sm.put(st, d_more, more.size, bad_chunks, more_dig)
        assert _code(ei) == c._lib.CDC_EINVAL, bad
        assert st.stats() == before
    # padded lengths whose 64-bit sum wraps to exactly 0 (no byte of such a buffer is read: refused first)
    with pytest.raises(c.CdcError) as ei:
        sm.put(st, d_more, 2 ** 63, np.array([[0, 2 ** 63], [0, 2 ** 63]], dtype=np.uint64), more_dig[:2])
    assert _code(ei) == c._lib.CDC_ENOMEM
    assert st.stats() == before
    dc, dg = sm.dev_chunks(more_chunks), sm.dev(more_dig)
    with pytest.raises(c.CdcError) as ei:  # chunk 19 = [1900, 100) of a stream declared 1999 long
        st.put_batch_device([d_more.data_ptr(), d_more.data_ptr() + 2000], [1999, 2000], [0, 20, 40],
                            dc.data_ptr(), dg.data_ptr())
    assert _code(ei) == c._lib.CDC_EINVAL
    assert st.stats() == before
    zero_based = more_chunks.copy()
    zero_based[20:, 0] -= 2000
    dc = sm.dev_chunks(zero_based)
    with pytest.raises(c.CdcError) as ei:  # the second stream's last chunk passes its lens[1]
        st.put_batch_device([d_more.data_ptr(), d_more.data_ptr() + 2000], [2000, 1999], [0, 20, 40],
                            dc.data_ptr(), dg.data_ptr())
    assert _code(ei) == c._lib.CDC_EINVAL
    assert st.stats() == before
    sm.get_checked(st, model, dig)
    assert st.put_batch_device([d_more.data_ptr(), d_more.data_ptr() + 2000], [2000, 2000], [0, 20, 40],
                               dc.data_ptr(), dg.data_ptr()) == 40


def test_clear():
    import chunkfs_amd as c
    st, model, dig = _small_store(c)
    st.clear()
    s = st.stats()
    assert all(s[k] == 0 for k in ("chunks_written", "bytes_written", "unique_chunks", "unique_bytes", "arena_used"))
    dd = sm.dev(dig[:1])
    with pytest.raises(c.CdcError) as ei:
        st.get_device(dd.data_ptr(), 1, None, 0)
    assert _code(ei) == c._lib.CDC_ENOTFOUND
    rng = np.random.default_rng(2)
    data = rng.integers(0, 256, 5000, dtype=np.uint8)
    chunks = np.array([[3, 1000], [1003, 1], [1500, 3333]], dtype=np.uint64)
    model = sm.Model()
    dig2, _ = model.put(data, chunks)
    assert sm.put(st, sm.dev(data), data.size, chunks, dig2).all()
    sm.assert_stats(st, model)  # arena_used counts from 0 again
    sm.get_checked(st, model, dig2[::-1])


def test_stream_order_on_a_user_stream():
    """fill -> chunk -> hash -> put -> get on one user stream with no host wait in between."""
    import torch
    import chunkfs_amd as c
    from chunkfs_amd import _lib
    n, seed = 1 << 20, 4242
    ch = c.FastChunker(c.SizeParams(4096, 8192, 16384))
    st = c.ChunkStore(1 << 10, 2 << 20)
    cap = ch.batch_max_chunks([n])
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.zeros((cap, 2), dtype=torch.int64, device="cuda")
    dig = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    _lib.check(_lib.lib().cdc_fill_splitmix64_device(ctypes.c_void_p(buf.data_ptr()), n, seed, ctypes.c_void_p(sp)))
    first = ch.chunk_batch_device([buf.data_ptr()], [n], out.data_ptr(), cap, stream=sp)
    k = int(first[1])
    ch.sha256_batch_device([buf.data_ptr()], first, out.data_ptr(), dig.data_ptr(), stream=sp)
    assert st.put_batch_device([buf.data_ptr()], [n], first, out.data_ptr(), dig.data_ptr(), stream=sp) == k
    assert st.get_device(dig.data_ptr(), k, back.data_ptr(), n, stream=sp) == n
    assert (back.cpu().numpy() == oracle.splitmix64_bytes(n, seed)).all()


def test_cpp_store_mirror_runs():
    from chunkfs_amd import _lib, build
    exe = os.path.join(ROOT, "_build", "store_example")
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
    assert "store ok: 2 new of 3, read 30 bytes" in r.stdout
