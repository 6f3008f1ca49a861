"""GPU suite of the per-store hasher (cdc_store_set_hash, include/chunkfs_amd.h):
a FileSystem(hash="blake2sp") through every call of the store and the file
layer that hashes -- the single write, the batch write, the splice, the unpack's
integrity check, the re-chunk scrub -- and through the calls that only carry
digests.  Digests are compared with the hashlib oracle of
tests/blake2sp_model.py over the chunk list of the FastCDC oracle; packs with the
image of tests/pack_model.py for the same table.  Files are 1-4 MiB."""
import struct
import types

import numpy as np
import pytest

import blake2sp_model as bm
import oracle
import pack_model as pm
import store_model as sm

pytestmark = pytest.mark.gpu
MB = 1 << 20
SIZES = (4096, 8192, 16384)
EINVAL = -1


def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def chunks_of(data):
    return oracle.fastcdc(data, *SIZES)


def new_fs(c, hash="blake2sp", **kw):  # noqa: A002
    kw.setdefault("max_chunks", 1 << 12)
    kw.setdefault("arena_bytes", 16 * MB)
    return c.FileSystem(hash=hash, **kw)


def chunker(c):
    return c.FastChunker(c.SizeParams(*SIZES))


def stats(fs):
    return {k: v for k, v in fs.store.stats().items() if v == v}


@pytest.fixture(scope="module")
def blob():
    """2 MiB of random bytes, its FastCDC chunk list and the BLAKE2sp digests, computed once."""
    data = rand(21, 2 * MB + 333)
    chunks = chunks_of(data)
    want = bm.digests(data, chunks)
    for a in (data, chunks, want):
        a.setflags(write=False)
    return data, chunks, want


def written(c, fs, ch, name, data):
    h = fs.create_file(name, ch)
    n = fs.write_to_file(h, data)
    return h, n


def test_write_to_file_hashes_with_blake2sp_and_reads_back(blob):
    import chunkfs_amd as c
    data, chunks, want = blob
    fs, ch = new_fs(c), chunker(c)
    assert fs.store.hash == "blake2sp"
    h, n = written(c, fs, ch, "f", data)
    assert n == len(chunks)
    assert (fs.hashes(h) == want).all()
    assert (fs.read_file_complete(h) == data).all()
    assert (fs.pread(h, 12345, 70000) == data[12345:82345]).all()
    d_data = sm.dev(data.copy())  # (the fixture's array is read-only, which torch warns about)
    ok, at = fs.verify_device(h, d_data.data_ptr(), data.size)
    assert ok and at is None
    # a duplicate file adds no arena bytes
    before = stats(fs)
    h2, n2 = written(c, fs, ch, "g", data)
    after = stats(fs)
    assert n2 == n and after["arena_used"] == before["arena_used"]
    assert after["unique_chunks"] == before["unique_chunks"] and after["bytes_written"] == 2 * before["bytes_written"]
    assert (fs.hashes(h2) == want).all()
    name = fs.get_to_dedup_ratio("f", 2.0)
    assert fs.file_exists(name) and stats(fs)["arena_used"] == before["arena_used"]


def test_write_to_files_in_one_batch(blob):
    import chunkfs_amd as c
    data, chunks, want = blob
    fs, ch = new_fs(c), chunker(c)
    other = rand(22, MB + 17)
    handles = [fs.create_file(n, ch) for n in ("a", "b", "c", "e")]
    datas = [data, other, np.zeros(0, dtype=np.uint8), data[:MB]]
    got = fs.write_to_files(handles, datas)
    for h, d, n in zip(handles, datas, got):
        ck = chunks_of(d) if d.size else np.zeros((0, 2), np.uint64)
        assert n == len(ck)
        assert (fs.hashes(h) == bm.digests(d, ck)).all()
        assert (fs.read_file_complete(h) == d).all()
    assert (fs.hashes(handles[0]) == want).all()


def test_store_write_hashes_with_the_stores_hasher():
    import chunkfs_amd as c
    data = rand(23, 300 * 1024 + 5)
    st, ch = c.ChunkStore(1 << 10, 4 * MB, hash="blake2sp"), chunker(c)
    ck, dig, new = st.write(ch, data)
    assert (dig == bm.digests(data, ck)).all() and new.all()
    assert (st.read(dig) == data).all()


@pytest.mark.parametrize("edit", ["pwrite", "insert", "delete_range"])
def test_edits_give_the_file_one_write_gives(blob, edit):
    import chunkfs_amd as c
    data = blob[0]
    fs, ch = new_fs(c), chunker(c)
    h, _ = written(c, fs, ch, "f", data)
    patch = rand(24, 4096)
    at = 777_777
    if edit == "pwrite":
        fs.pwrite(h, at, patch)
        new = np.concatenate([data[:at], patch, data[at + patch.size:]])
    elif edit == "insert":
        fs.insert(h, at, patch)
        new = np.concatenate([data[:at], patch, data[at:]])
    else:
        fs.delete_range(h, at, 5000)
        new = np.concatenate([data[:at], data[at + 5000:]])
    ck = chunks_of(new)
    assert fs.stat(h)["spans"] == len(ck)
    assert (fs.hashes(h) == bm.digests(new, ck)).all()  # span for span the file one write gives
    assert (fs.read_file_complete(h) == new).all()
    twin = new_fs(c)
    ht, _ = written(c, twin, ch, "f", new)
    assert (twin.hashes(ht) == fs.hashes(h)).all()


def test_clone_diff_remove_and_collect(blob):
    import chunkfs_amd as c
    data, chunks, want = blob
    fs, ch = new_fs(c), chunker(c)
    h, n = written(c, fs, ch, "f", data)
    before = stats(fs)
    assert fs.clone_file("f", "g") == n and stats(fs) == before
    g = fs.open_file("g", ch)
    assert fs.diff(h, g).n_ranges == 0
    patch = rand(25, 4096)
    fs.pwrite(g, MB, patch)
    d = fs.diff(h, g)
    lo, hi = int(d.ranges[0, 0]), int(d.ranges[-1, 0] + d.ranges[-1, 1])
    assert d.n_ranges >= 1 and MB <= lo and hi <= MB + 4096
    assert (fs.hashes(h) == want).all()
    fs.remove_file("f")
    r = fs.collect()
    assert r["containers_after"] == len({bytes(x) for x in fs.hashes(g)}) < r["containers_before"]
    new = np.concatenate([data[:MB], patch, data[MB + 4096:]])
    assert (fs.read_file_complete(g) == new).all()
    assert (fs.hashes(g) == bm.digests(new, chunks_of(new))).all()


def test_rechunk_scrub_hashes_the_sub_chunks_with_blake2sp():
    import hashlib

    import torch

    import chunkfs_amd as c
    data = rand(26, MB + 99)
    ch, sub = chunker(c), c.FSChunker(512)
    fs = c.FileSystem.new_with_scrubber(c.RechunkScrubber(sub), max_chunks=1 << 10, arena_bytes=4 * MB,
                                        target_max_chunks=1 << 13, target_arena_bytes=4 * MB, hash="blake2sp")
    assert fs.store.hash == "blake2sp" and fs.target.hash == "blake2sp"
    h, _ = written(c, fs, ch, "f", data)
    m = fs.scrub()
    assert m.processed_data == data.size
    assert (fs.read_file_complete(h) == data).all()
    assert (fs.pread(h, 5000, 3000) == data[5000:8000]).all()
    # the target map's keys are the BLAKE2sp digests of the 512-byte sub-chunks
    first = int(chunks_of(data)[0, 1])
    pieces = [data[o:min(o + 512, first)].tobytes() for o in range(0, first, 512)]
    keys = np.stack([np.frombuffer(bm.oracle(p), dtype=np.uint8) for p in pieces] +
                    [np.frombuffer(hashlib.sha256(p).digest(), dtype=np.uint8) for p in pieces])
    d = torch.from_numpy(keys).cuda()
    found = torch.zeros(len(keys), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fs.target.contains_device(d.data_ptr(), len(keys), found.data_ptr())
    found = found.cpu().numpy().astype(bool)
    assert found[:len(pieces)].all() and not found[len(pieces):].any()
    subs = [(o, min(512, s + n - o)) for s, n in chunks_of(data).tolist() for o in range(s, s + n, 512)]
    assert fs.store.scrub_stats()["target_values"] == len({bytes(k) for k in bm.digests(data, subs)})


class Table:
    """What pack_model.pack reads of a files model: the spans and the chunk bytes."""

    def __init__(self, data, chunks, digests):
        self.spans = [types.SimpleNamespace(hash=bytes(d), len=int(n)) for d, (_, n) in zip(digests, chunks.tolist())]
        self.store = types.SimpleNamespace(db={bytes(d): data[int(o):int(o) + int(n)].tobytes()
                                               for d, (o, n) in zip(digests, chunks.tolist())})

    def _spans(self, h):
        return self.spans


def flags_of(pack):
    return struct.unpack_from("<I", pack, 12)[0]


def test_pack_and_unpack_between_two_blake2sp_stores(blob):
    import chunkfs_amd as c
    data, chunks, want = blob
    a, b, ch = new_fs(c), new_fs(c), chunker(c)
    h, _ = written(c, a, ch, "f", data)
    t, st = a.pack(h)
    pack = t.cpu().numpy().tobytes()
    image, wst = pm.pack(Table(data, chunks, want), None)
    assert flags_of(pack) == 1 and flags_of(image) == 0
    assert pack[:12] == image[:12] and pack[16:] == image[16:]  # all but the flags word
    assert {k: getattr(st, k) for k in pm.STATS} == wst
    got = b.unpack("f", t, hasher=ch)
    assert got.chunks_new == st.chunks
    assert stats(a) == stats(b)
    hb = b.open_file("f", ch)
    assert (b.hashes(hb) == want).all() and (b.read_file_complete(hb) == data).all()
    # a corrupted data byte is refused, before anything is written
    bad = bytearray(pack)
    _, _, _, _, _, _, _, data_bytes, total = pm.HEADER.unpack_from(pack, 0)
    bad[total - data_bytes] ^= 1  # the first byte of the first carried chunk
    e = new_fs(c)
    with pytest.raises(c.CdcError) as x:
        e.unpack("f", np.frombuffer(bytes(bad), dtype=np.uint8), hasher=ch)
    assert x.value.code == EINVAL and "does not hash to its digest" in str(x.value)
    assert e.list_files() == [] and stats(e)["unique_chunks"] == 0
    # send between the two, with the check
    sent, recv = a.send(h, b, name="again", hasher=ch)
    assert sent.chunks == 0 and recv.external_spans == len(chunks)


@pytest.mark.parametrize("src,dst", [("blake2sp", "sha256"), ("sha256", "blake2sp")])
def test_a_pack_into_a_store_with_another_hasher_is_refused(src, dst):
    import chunkfs_amd as c
    data = rand(27, MB)
    a, b, ch = new_fs(c, hash=src), new_fs(c, hash=dst), chunker(c)
    h, _ = written(c, a, ch, "f", data)
    hk, _ = written(c, b, ch, "kept", data[:300_000])
    before = stats(b), b.list_files()
    t, _ = a.pack(h)
    assert flags_of(t.cpu().numpy().tobytes()) == (1 if src == "blake2sp" else 0)
    for trust in (False, True):
        with pytest.raises(c.CdcError) as x:
            b.unpack("f", t, hasher=None if trust else ch, trust=trust)
        assert x.value.code == EINVAL and "flags" in str(x.value)
        assert (stats(b), b.list_files()) == before
    with pytest.raises(c.CdcError) as x:
        a.send(h, b, hasher=ch)
    assert x.value.code == EINVAL and "flags" in str(x.value)
    assert (stats(b), b.list_files()) == before
    assert (b.read_file_complete(hk) == data[:300_000]).all()


def test_set_hash_rules():
    import chunkfs_amd as c
    st, ch = c.ChunkStore(1 << 8, MB), chunker(c)
    assert st.hash == "sha256"
    st.set_hash("blake2sp")
    st.set_hash("sha256")
    st.write(ch, rand(28, 50_000))
    with pytest.raises(c.CdcError) as x:
        st.set_hash("blake2sp")
    assert x.value.code == EINVAL and "holds chunks" in str(x.value) and st.hash == "sha256"
    st.clear()
    st.set_hash("blake2sp")  # allowed again
    assert st.hash == "blake2sp"
    with pytest.raises(c.CdcError) as x:
        st.set_hash(2)
    assert x.value.code == EINVAL and "unknown hasher" in str(x.value) and st.hash == "blake2sp"
    # two stores with different hashers cannot be attached
    target = c.ChunkStore(1 << 8, MB)
    with pytest.raises(c.CdcError) as x:
        st.set_target(target)
    assert x.value.code == EINVAL and "different hashers" in str(x.value)
    target.set_hash("blake2sp")
    st.set_target(target)
    for s, words in ((st, "a target store is attached"), (target, "another store's target")):
        with pytest.raises(c.CdcError) as x:
            s.set_hash("sha256")
        assert x.value.code == EINVAL and words in str(x.value) and s.hash == "blake2sp"
    with pytest.raises(ValueError):
        c.FileSystem(store=st, hash="sha256")
    del st  # the base before its target


def test_a_default_file_system_still_packs_with_flags_0(blob):
    import hashlib

    import chunkfs_amd as c
    data, chunks, _ = blob
    fs, ch = c.FileSystem(max_chunks=1 << 12, arena_bytes=16 * MB), chunker(c)
    assert fs.store.hash == "sha256"
    h, _ = written(c, fs, ch, "f", data)
    sha = np.stack([np.frombuffer(hashlib.sha256(data[int(o):int(o) + int(n)].tobytes()).digest(), dtype=np.uint8)
                    for o, n in chunks.tolist()])
    assert (fs.hashes(h) == sha).all()
    t, _ = fs.pack(h)
    pack = t.cpu().numpy().tobytes()
    assert flags_of(pack) == 0 and pack == pm.pack(Table(data, chunks, sha), None)[0]
