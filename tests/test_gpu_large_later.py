"""The later features past the 4 GiB line (-m gpu): the batch write, BLAKE2sp,
packs and the content-aligned delta on the stream, the file and the arena of
tests/test_gpu_large.py -- N_BIG = 2^32 + 16 MiB + 4099 bytes -- with that
module's plumbing (Big, make, Guard, pread_checked, slots_of) and its method:
one device buffer, closed-form expectations, comparisons on the device.  Every
comparison is exact.  Expected values come from the host copy of the stream
with numpy and hashlib (tests/large_model.py: blake2sp_rows, pack_index, the
delta closed forms; tests/test_large_model.py proves each against the model of
its feature at small sizes, and that at N_BIG each holds a value >= 2^32 which
32 bits would change); none is taken from the code under test.

What each case reaches past 2^32:

  A batch write  first[] and the per-request bases of cdc_files_write_batch_device
                 after a 4 GiB request; the append of a batch whose span offsets
                 cross the line; put_batch's locs past the line
  B BLAKE2sp     `src = base + offset` past 2^32 in hash_feed.hpp's load_window;
                 the order[] claim over 2^19 chunks (the 4/8/16 KiB list); the
                 same list as 64 streams whose offsets all lie below 2^32; a
                 store keyed by BLAKE2sp digests with loc >= 2^32, and the
                 verify kernel over it
  C packs        PackLayout's section offsets, chunk_off[] and data_bytes past
                 2^32; the copy's tile bound data_bytes / kStoreTile + n_chunks
                 (> 2^18); StorePiece sources at arena + loc, loc >= 2^32 (and
                 >= N_BIG: `late`); the hash of pack chunks at offsets past 2^32
                 in the pack buffer and the mismatch index of one of them;
                 PackSum over lengths that sum past 2^32; an incremental pack
                 whose externals are looked up in a store filled past the line
  D delta        COPY ops with a_off >= 2^32 and b_off >= 2^32; diagonals above
                 2^32 and below -2^32; one LITERAL longer than 2^32 bytes, whose
                 region has more than kDlMaxBlocks = 2^18 tiles, so that the edge
                 kernel's stride loop makes a second pass (no smaller case can);
                 the `acc` byte sums past 2^32; the nearest-offset search between
                 two occurrences of a slot more than 2^32 apart

Out of scope: packs with `have` (the same kernels, one more bit per slot); the
host-buffer paths (save_file / load_file and host `datas` of write_to_files:
their staging copies dominate); send between two devices; more than one GPU.

The BLAKE2sp cases use the 32 / 128 / 1024 KiB list: hashlib's blake2s runs at
a third of its SHA-256's speed, and the 8 KiB leaves of a 64 KiB chunk are too
short for the threads to overlap (256 MiB of 64 KiB chunks took 8 threads as
long as one, 0.43 s; of 512 KiB chunks a third of that), which puts the oracle
over the 16 / 64 / 256 KiB list near 15 s against 2 s here.  Every row of the
list is compared.

Device memory at any moment: the buffer 4.1 GiB; case A two arenas of N_BIG +
64 MiB and the N_BIG read-back buffer; case B one arena of N_BIG + 64 MiB; cases
C the `src` arena of N_BIG + 1 GiB, one pack of 4.2 GiB, the `dst` arena of
N_BIG + 64 MiB and 2 GiB of index tensors for the data section's comparison;
case D the `src` arena and two tensors of N_BIG for apply_delta's answer and the
read-back.  Long tensors are compared a GiB at a time (same_bytes): torch.equal
of two 4 GiB tensors takes another 4 GiB.  The module skips only when the
device reports less free memory than NEED_FREE, which is derived below from
the measured peak.

Wall times measured on an MI355X host, hashlib and the oracle on 16 CPU
threads.  The fixtures: device fill and host copy as in test_gpu_large; hashlib
SHA-256 of the 16/64/256 KiB list 0.40 s; hashlib BLAKE2sp of the 27042 chunks
of the 32/128/1024 KiB list 1.61 s; the write of `filler` 0.02 s.  The cases:

  A batch write 0.84 s with the SHA-256 fixture: the oracle over the list
    0.07 s, write_to_files 0.03 s, three write_to_file 0.04 s, reads + hashes +
    verify of six files 0.34 s
  B one stream 0.01 s (the call 0.01 s); half a million chunks as one stream
    and as 64, with hashlib on 1800 rows, 0.12 s; the BLAKE2sp store 0.16 s
  C full pack 0.56 s (the pack itself under 0.01 s, the index and the data
    section compared in 0.45 s); unpack 0.09 s (the call 0.02 s, the refused
    one 0.02 s); incremental pack and unpack 0.01 s; pack of `late` 0.02 s
  D insert 0.44 s (the delta under 0.01 s, apply_delta 0.36 s); dropped head
    and back 0.03 s (0.02 s and under 0.01 s); a slot twice 0.02 s; truncation
    and back under 0.01 s
  the whole module 5.5 s (7.8 s with pytest's own), 12 passed, none skipped;
  device memory in use peaked at 20.0 GiB, in the full pack's comparison
  (0.6 GiB of it before the module began)
"""
import gc
import re
import struct
import time

import numpy as np
import pytest

import large_model as lm
import oracle
import pack_model as pm
from large_model import LINE, N_BIG
from test_gpu_large import (DEV, EDIT_AT, EDIT_N, LATE_N, MIB, S4, S_BIG, S_STORE, SEED, Big, Guard, make,
                            pread_checked, slots_of)

pytestmark = pytest.mark.gpu

GIB = 1 << 30
S_B2 = S_BIG                               # the BLAKE2sp cases' list (see the docstring)
SRC_ARENA, DST_ARENA = N_BIG + GIB, N_BIG + (64 << 20)
REALIGN = 16 * S_STORE[2]                  # test_gpu_large's bound on what one edit re-chunks: 16 max-size chunks
LIT = lm.DELTA_LIT
# The budget.  By the plan the largest moment is the full pack's comparison: buffer, `src` arena, pack, `dst`
# arena and 2 GiB of index tensors for a slab.  MEASURED_PEAK is the most a run reported as in use (see the
# docstring), MEASURED_BEFORE what was in use before the module began; 2 GiB of slack for the allocators'
# rounding.  Under the 24 GiB test_gpu_large asks for.
PLAN = N_BIG + SRC_ARENA + (N_BIG + (80 << 20)) + DST_ARENA + 2 * GIB
MEASURED_PEAK, MEASURED_BEFORE = 20.0, 0.6
NEED_FREE = int((MEASURED_PEAK - MEASURED_BEFORE + 2.0) * GIB)
assert PLAN <= NEED_FREE <= 24 * GIB
PEAK = {"gib": 0.0}


# ---- plumbing ---------------------------------------------------------------------

def mem(torch):
    """Device memory in use now, GiB; the module's peak is the largest seen."""
    free, total = torch.cuda.mem_get_info()
    used = (total - free) / GIB
    PEAK["gib"] = max(PEAK["gib"], used)
    return used


def release(torch):
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big():
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip(f"test_gpu_large_later needs {NEED_FREE >> 30} GiB of free device memory; {free >> 20} MiB are free")
    t0 = time.perf_counter()
    base = mem(torch)
    b = Big(torch)
    yield b
    b._lists.clear()
    b._scratch = b.buf = b.host = None
    del b
    release(torch)
    print(f"\n[later] the whole module {time.perf_counter() - t0:.1f} s; device memory in use peaked at "
          f"{PEAK['gib']:.1f} GiB ({base:.1f} GiB of it before the module began)")


@pytest.fixture(autouse=True)
def _report(request):
    import torch
    t0 = time.perf_counter()
    yield
    print(f"\n[later] {request.node.name}: {time.perf_counter() - t0:.2f} s, device memory in use {mem(torch):.1f} GiB, "
          f"peak so far {PEAK['gib']:.1f} GiB")


def lap(what, t0):
    print(f"\n[later]   {what}: {time.perf_counter() - t0:.2f} s")
    return time.perf_counter()


def store_stats(fs):
    s = fs.store.stats()
    return {k: s[k] for k in ("unique_chunks", "unique_bytes", "chunks_written", "bytes_written", "arena_used")}


def table_of(big, fs, h):
    """(the file's bytes in the shared read-back buffer, its span table on the host)."""
    import torch
    st = fs.stat(h)
    back = big.scratch()
    d_spans = torch.full((max(st["spans"], 1), 2), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    assert fs.read_complete_device(h, back.data_ptr(), N_BIG, d_spans.data_ptr()) == st["size"]
    torch.cuda.synchronize()
    return back[:st["size"]], d_spans[:st["spans"]].cpu().numpy().view(np.uint64)


def same_bytes(torch, x, y, slab=GIB):
    """torch.equal of two long uint8 tensors, a slab at a time (its temporary stays small)."""
    return x.numel() == y.numel() and all(torch.equal(x[a:a + slab], y[a:a + slab]) for a in range(0, x.numel(), slab))


def ops_of(r):
    return [tuple(int(x) for x in o) for o in r.ops.tolist()]


def distinct(digests):
    return len(np.unique(np.ascontiguousarray(digests).view("<u8").reshape(-1, 4), axis=0)) == len(digests)


@pytest.fixture(scope="module")
def sha_store(big):
    """hashlib SHA-256 of the 16 / 64 / 256 KiB list (shared, read-only)."""
    t0 = time.perf_counter()
    d = lm.sha256_rows(big.host, big.chunks("fast", S_STORE)[1])
    d.setflags(write=False)
    lap("hashlib sha256 of the 16/64/256 KiB list", t0)
    return d


# ---- A. the batch write -------------------------------------------------------------

SMALL = ((3 * MIB + 17, 81), (MIB + 13, 82))


def test_batch_write_around_a_huge_file(big, sha_store):
    import torch
    import chunkfs_amd as c
    whole = big.chunks("fast", S_STORE)[1]
    t0 = time.perf_counter()
    big.verify(whole, "fast", S_STORE, f"fastcdc {S_STORE}")                 # the list itself, against the oracle
    t0 = lap("oracle over the 16/64/256 KiB list", t0)
    hosts = [oracle.splitmix64_bytes(n, seed) for n, seed in SMALL]
    devs = [torch.from_numpy(x).to(DEV) for x in hosts]
    want_rows = [oracle.fastcdc(hosts[0], *S_STORE), whole, oracle.fastcdc(hosts[1], *S_STORE)]
    want_dig = [lm.sha256_rows(hosts[0], want_rows[0]), sha_store, lm.sha256_rows(hosts[1], want_rows[2])]
    sizes = [hosts[0].size, N_BIG, hosts[1].size]
    datas = [devs[0], big.buf, devs[1]]
    assert len(want_rows[0]) > 10 and len(want_rows[2]) > 3 and sizes[0] + N_BIG >= LINE
    ch = make("fast", S_STORE)
    kw = dict(max_chunks=1 << 18, arena_bytes=DST_ARENA)
    one, three = c.FileSystem(**kw), c.FileSystem(**kw)
    names = ("small0", "huge", "small1")
    h1 = [one.create_file(n, ch) for n in names]
    h3 = [three.create_file(n, ch) for n in names]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counts = one.write_to_files(h1, datas)
    t0 = lap("write_to_files", t0)
    singles = [three.write_to_file(h, d) for h, d in zip(h3, datas)]
    t0 = lap("three write_to_file", t0)
    mem(torch)
    assert counts == singles == [len(r) for r in want_rows]
    assert store_stats(one) == store_stats(three)
    n_all, padded = sum(counts), sum(int(lm.pad16(r[:, 1]).sum()) for r in want_rows)
    assert store_stats(one) == {"unique_chunks": n_all, "unique_bytes": sum(sizes), "chunks_written": n_all,
                                "bytes_written": sum(sizes), "arena_used": padded}
    for i in range(3):
        for fs, h in ((one, h1[i]), (three, h3[i])):
            st = fs.stat(h)
            assert (st["size"], st["spans"]) == (sizes[i], counts[i]), (names[i], st)
            body, table = table_of(big, fs, h)
            assert np.array_equal(table, want_rows[i]), names[i]
            assert same_bytes(torch, body, datas[i]), names[i]
            mem(torch)
            assert np.array_equal(fs.hashes(h), want_dig[i]), names[i]
        assert slots_of(one, h1[i])[1] == slots_of(three, h3[i])[1]        # the same arena, byte for byte
    assert max(slots_of(one, h1[1])[1]) >= LINE and min(slots_of(one, h1[2])[1]) >= N_BIG
    assert one.verify_device(h1[1], big.buf.data_ptr(), N_BIG) == (True, None)
    g = Guard(sizes[2], 3)
    g.check(one.read_complete_device(h1[2], g.ptr, sizes[2]), hosts[1], "small1, whole")
    pread_checked(one, h1[1], LINE - 4097, 8195, big.host[LINE - 4097:LINE + 4098], 5)
    lap("the comparisons", t0)
    del one, three, h1, h3, g, body, fs, h
    ch.close()
    big._scratch = None
    release(torch)


# ---- B. BLAKE2sp ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def b2_rows(big):
    """hashlib BLAKE2sp of every chunk of the S_B2 list (shared, read-only)."""
    whole = big.chunks("fast", S_B2)[1]
    t0 = time.perf_counter()
    d = lm.blake2sp_rows(big.host, whole)
    d.setflags(write=False)
    lap(f"hashlib blake2sp of the {len(whole)} chunks of the {S_B2} list", t0)
    return d


def device_digests(torch, ch, ptrs, first, d_chunks, n):
    dig = torch.full((n + 1, 32), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    ch.hash_batch_device(ptrs, first, d_chunks.data_ptr(), dig.data_ptr(), hash="blake2sp")
    torch.cuda.synchronize()
    assert bool((dig[n] == 0xA5).all()), "a digest was written past the last chunk's row"
    return dig[:n]


def assert_digests(got, want, rows, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (f"{what}: {len(bad)} of {len(want)} digests wrong, first at chunk {int(bad[0])} "
                          f"[offset, length] {[int(x) for x in rows[bad[0]]]}")


def test_blake2sp_whole_list_as_one_stream(big, b2_rows):
    import torch
    d_list, whole = big.chunks("fast", S_B2)
    n = len(whole)
    assert n > 8000 and int(whole[-1, 0]) >= LINE
    ch = make("fast", S_B2)
    t0 = time.perf_counter()
    got = device_digests(torch, ch, [big.buf.data_ptr()], [0, n], d_list, n)
    lap("hash_batch_device", t0)
    ch.close()
    assert_digests(got.cpu().numpy(), b2_rows, whole, "blake2sp, one stream")


def test_blake2sp_half_a_million_chunks_one_stream_and_64(big):
    import torch
    d_list, whole = big.chunks("fast", S4)
    n = len(whole)
    assert n > 1 << 18
    ch = make("fast", S4)
    t0 = time.perf_counter()
    one = device_digests(torch, ch, [big.buf.data_ptr()], [0, n], d_list, n)
    t0 = lap("one stream", t0)
    k = lm._boundary_rows(whole, N_BIG, 64)
    assert len(k) == 64 and k[0] == 0
    first = [int(x) for x in k] + [n]
    start = whole[k, 0]
    rel = whole.copy()
    rel[:, 0] -= np.repeat(start, np.diff(first))
    assert int(rel[:, 0].max()) < LINE < int(whole[:, 0].max()) and int((rel[:, 0] + rel[:, 1]).max()) < 1 << 27
    d_rel = torch.from_numpy(rel.view(np.int64)).to(DEV)
    ptrs = [big.buf.data_ptr() + int(s) for s in start]
    many = device_digests(torch, ch, ptrs, first, d_rel, n)
    lap("64 streams", t0)
    ch.close()
    assert torch.equal(one, many)
    # ... and hashlib on the rows around the line and at both ends (all of them are compared in the case above,
    # on the longer chunks of the other list)
    a = int(np.searchsorted(whole[:, 0], np.uint64(LINE))) - 600
    got = one.cpu().numpy()
    for lo, hi in ((0, 300), (a, a + 1200), (n - 300, n)):
        assert_digests(got[lo:hi], lm.blake2sp_rows(big.host, whole[lo:hi]), whole[lo:hi], f"rows {lo}..{hi}")


def test_blake2sp_store_takes_the_stream_in_one_write(big, b2_rows):
    import torch
    import chunkfs_amd as c
    whole = big.chunks("fast", S_B2)[1]
    n = len(whole)
    ch = make("fast", S_B2)
    fs = c.FileSystem(max_chunks=1 << 17, arena_bytes=DST_ARENA, hash="blake2sp")
    h = fs.create_file("filler", ch)
    t0 = time.perf_counter()
    assert fs.write_to_file(h, big.buf) == n
    lap("write_to_file, blake2sp", t0)
    mem(torch)
    st = fs.stat(h)
    assert (st["size"], st["spans"]) == (N_BIG, n)
    assert distinct(b2_rows)
    assert store_stats(fs) == {"unique_chunks": n, "unique_bytes": N_BIG, "chunks_written": n, "bytes_written": N_BIG,
                               "arena_used": int(lm.pad16(whole[:, 1]).sum())}
    assert max(slots_of(fs, h)[1]) >= LINE
    assert_digests(fs.hashes(h), b2_rows, whole, "hashes() of the blake2sp layer")
    assert fs.verify_device(h, big.buf.data_ptr(), N_BIG) == (True, None)
    pread_checked(fs, h, LINE - 70001, 140003, big.host[LINE - 70001:LINE + 70002], 3)
    try:
        big.buf[LINE + 7] ^= 0x40
        torch.cuda.synchronize()
        assert fs.verify_device(h, big.buf.data_ptr(), N_BIG) == (False, LINE + 7)
    finally:
        big.buf[LINE + 7] ^= 0x40
        torch.cuda.synchronize()
    assert fs.verify_device(h, big.buf.data_ptr(), N_BIG) == (True, None)
    assert fs.write_to_file(h, big.buf[:S_B2[2] * 4]) > 0                    # every chunk but the last is known:
    after = store_stats(fs)                                                  # looked up by digest, loc untouched
    assert after["unique_chunks"] <= n + 1 and after["chunks_written"] > n
    del fs, h
    ch.close()
    release(torch)


# ---- C. packs -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def src(big):
    """TestFiles.fsys of test_gpu_large: `filler` holds the stream, `late` lies behind it in the arena."""
    import torch
    import chunkfs_amd as c
    ch = make("fast", S_STORE)
    fs = c.FileSystem(max_chunks=1 << 20, arena_bytes=SRC_ARENA)
    filler = fs.create_file("filler", ch)
    t0 = time.perf_counter()
    spans = fs.write_to_file(filler, big.buf)
    lap("write of filler", t0)
    late_data = oracle.splitmix64_bytes(LATE_N, SEED + 1)
    late = fs.create_file("late", ch)
    fs.write_to_file(late, late_data)
    assert spans == len(big.chunks("fast", S_STORE)[1])
    state = {"fs": fs, "ch": ch, "filler": filler, "late": late, "late_data": late_data}
    yield state
    state.clear()
    del fs, filler, late
    ch.close()
    release(torch)


@pytest.fixture(scope="module")
def dst(big):
    import torch
    import chunkfs_amd as c
    state = {"fs": c.FileSystem(max_chunks=1 << 18, arena_bytes=DST_ARENA), "pack": None, "index": None}
    yield state
    state.clear()
    release(torch)


def header_of(pack):
    return struct.unpack("<8sIIQQQQQQ", pack[:64].cpu().numpy().tobytes())


def assert_index(torch, pack, x, what):
    """Everything before the data section, bit for bit."""
    want = torch.from_numpy(x.index).to(DEV)
    got = pack[:x.layout["data"]]
    if not torch.equal(got, want):
        at = int(torch.nonzero(got != want)[0, 0])
        section = [k for k, v in x.layout.items() if v <= at][-1] if at >= 64 else "header"
        raise AssertionError(f"{what}: the pack differs from the expected index at byte {at} ({section} section)")


def test_full_pack_of_the_stream(big, sha_store, src, dst):
    import torch
    fs, filler = src["fs"], src["filler"]
    whole = big.chunks("fast", S_STORE)[1]
    n = len(whole)
    assert distinct(sha_store)                                   # so that every span carries its own chunk
    x = lm.pack_index(whole, sha_store)
    data_bytes = int(lm.pad16(whole[:, 1]).sum())
    lay = pm.layout(n, n, data_bytes)
    assert x.n_chunks == n and x.data_bytes == data_bytes and x.layout == lay
    assert int(x.chunk_off[-2]) >= LINE and lay["total"] > data_bytes > N_BIG
    assert max(slots_of(fs, filler)[1]) >= LINE
    t0 = time.perf_counter()
    pack, st = fs.pack(filler)
    t0 = lap("pack", t0)
    mem(torch)
    assert pack.numel() == lay["total"]
    assert {k: getattr(st, k) for k in pm.STATS} == {"spans": n, "chunks": n, "external_spans": 0, "chunk_bytes": N_BIG,
                                                      "pack_bytes": lay["total"], "file_size": N_BIG, "chunks_new": 0}
    assert header_of(pack) == (pm.MAGIC, 1, 0, N_BIG, n, n, 0, data_bytes, lay["total"])
    assert_index(torch, pack, x, "full pack")
    bad = lm.pack_data_mismatch(pack[lay["data"]:], big.buf, whole, x.chunk_span, x.chunk_off)
    mem(torch)
    assert bad is None, f"the data section differs at its byte {bad}"
    lap("the comparisons", t0)
    dst["pack"], dst["index"] = pack, x
    release(torch)


def test_unpack_of_the_full_pack(big, sha_store, src, dst):
    import torch
    import chunkfs_amd as c
    to, pack, x = dst["fs"], dst["pack"], dst["index"]
    assert pack is not None, "needs test_full_pack_of_the_stream"
    whole = big.chunks("fast", S_STORE)[1]
    n, lay = len(whole), x.layout
    t0 = time.perf_counter()
    st = to.unpack("filler", pack, hasher=src["ch"])
    t0 = lap("unpack", t0)
    mem(torch)
    assert {k: getattr(st, k) for k in pm.STATS} == {"spans": n, "chunks": n, "external_spans": 0, "chunk_bytes": N_BIG,
                                                      "pack_bytes": lay["total"], "file_size": N_BIG, "chunks_new": n}
    h = to.open_file_readonly("filler")
    stat = to.stat(h)
    assert (stat["size"], stat["spans"]) == (N_BIG, n)
    assert store_stats(to) == {"unique_chunks": n, "unique_bytes": N_BIG, "chunks_written": n, "bytes_written": N_BIG,
                               "arena_used": x.data_bytes}
    assert np.array_equal(to.hashes(h), sha_store)
    assert to.verify_device(h, big.buf.data_ptr(), N_BIG) == (True, None)
    assert max(slots_of(to, h)[1]) >= LINE
    pread_checked(to, h, LINE - 5003, 10007, big.host[LINE - 5003:LINE + 5004], 7)
    pread_checked(to, h, N_BIG - 100, 150, big.host[N_BIG - 100:], 1)
    t0 = lap("the comparisons", t0)

    # one flipped byte in a chunk that begins past 2^32 in the data section
    k = int(np.searchsorted(x.chunk_off, np.uint64(LINE)))
    at = lay["data"] + int(x.chunk_off[k]) + 1
    assert int(x.chunk_off[k]) >= LINE and k < n - 1 and int(whole[int(x.chunk_span[k]), 1]) > 1
    before, files = store_stats(to), to.list_files()
    try:
        pack[at] ^= 0x40
        torch.cuda.synchronize()
        with pytest.raises(c.CdcError) as e:
            to.unpack("damaged", pack, hasher=src["ch"])
    finally:
        pack[at] ^= 0x40
        torch.cuda.synchronize()
    assert e.value.code == c._lib.CDC_EINVAL
    m = re.search(r"carried chunk (\d+) does not hash to its digest \((\d+) in all\)", str(e.value))
    assert m and (int(m.group(1)), int(m.group(2))) == (k, 1), str(e.value)
    assert store_stats(to) == before and to.list_files() == files == ["filler"]
    lap("the refused unpack", t0)
    dst["pack"] = None
    del pack
    release(torch)


def test_incremental_pack_after_an_edit_past_the_line(big, src, dst):
    import torch
    fs, ch, filler, to, host = src["fs"], src["ch"], src["filler"], dst["fs"], big.host
    assert to.list_files() == ["filler"], "needs test_unpack_of_the_full_pack"
    n_before = fs.stat(filler)["spans"]
    assert fs.clone_file("filler", "snap") == n_before
    snap = fs.open_file_readonly("snap")
    new = host[EDIT_AT:EDIT_AT + EDIT_N] ^ np.uint8(0xFF)

    def edited(a, b):
        w = host[a:b].copy()
        lo, hi = max(a, EDIT_AT), min(b, EDIT_AT + EDIT_N)
        if lo < hi:
            w[lo - a:hi - a] = new[lo - EDIT_AT:hi - EDIT_AT]
        return w

    try:
        s = fs.pwrite(filler, EDIT_AT, new)
        assert (s.size_before, s.size_after) == (N_BIG, N_BIG)
        n = fs.stat(filler)["spans"]
        t0 = time.perf_counter()
        pack, st = fs.pack(filler, since=snap)
        t0 = lap("pack since the snapshot", t0)
        # The carried chunks are the spans the splice re-chunked: new bytes, so slots `snap` does not name.  The
        # bound is test_gpu_large's: cuts realign within a few chunks, 16 max-size chunks is far more than that.
        assert EDIT_N <= st.chunk_bytes <= REALIGN and 1 <= st.chunks <= REALIGN // S_STORE[0]
        assert (st.spans, st.external_spans, st.file_size, st.chunks_new) == (n, n - st.chunks, N_BIG, 0)
        hdr = header_of(pack)
        data_bytes = hdr[7]
        assert st.chunk_bytes <= data_bytes < st.chunk_bytes + 16 * st.chunks and data_bytes % 16 == 0
        total = pm.layout(n, st.chunks, data_bytes)["total"]
        assert hdr == (pm.MAGIC, 1, 0, N_BIG, n, st.chunks, n - st.chunks, data_bytes, total)
        assert st.pack_bytes == pack.numel() == total < REALIGN + 64 * n + 4096
        before = store_stats(to)
        got = to.unpack("edited", pack, hasher=ch)
        lap("unpack of the increment", t0)
        assert (got.spans, got.chunks, got.external_spans, got.chunk_bytes, got.pack_bytes, got.file_size,
                got.chunks_new) == (n, st.chunks, n - st.chunks, st.chunk_bytes, total, N_BIG, st.chunks)
        after = store_stats(to)
        assert after == {"unique_chunks": before["unique_chunks"] + st.chunks,
                         "unique_bytes": before["unique_bytes"] + st.chunk_bytes,
                         "chunks_written": before["chunks_written"] + n,
                         "bytes_written": before["bytes_written"] + N_BIG,
                         "arena_used": before["arena_used"] + data_bytes}
        h = to.open_file_readonly("edited")
        stat = to.stat(h)
        assert (stat["size"], stat["spans"]) == (N_BIG, n)
        a = EDIT_AT - 70000
        pread_checked(to, h, a, 150000, edited(a, a + 150000), 3)
        pread_checked(to, h, 0, 65536, host[:65536], 1)
        pread_checked(to, h, N_BIG - 65536, 65536 + 9, host[N_BIG - 65536:], 5)
        pread_checked(to, h, LINE - 33, 67, host[LINE - 33:LINE + 34], 2)
        assert to.verify_device(h, big.buf.data_ptr(), N_BIG) == (False, EDIT_AT)
        old = to.open_file_readonly("filler")                                       # the base is as it was
        assert to.verify_device(old, big.buf.data_ptr(), N_BIG) == (True, None)
    finally:
        fs.pwrite(filler, EDIT_AT, host[EDIT_AT:EDIT_AT + EDIT_N])                   # the later cases read `filler`
    assert fs.verify_device(filler, big.buf.data_ptr(), N_BIG) == (True, None)
    assert fs.diff(snap, filler).ranges.tolist() == []
    mem(torch)


def test_pack_of_a_file_behind_the_stream_in_the_arena(big, src, dst):
    import torch
    fs, late, data, to = src["fs"], src["late"], src["late_data"], dst["fs"]
    locs = slots_of(fs, late)[1]
    assert len(locs) == fs.stat(late)["spans"] and min(locs) >= N_BIG
    rows = oracle.fastcdc(data, *S_STORE)
    x = lm.pack_index(rows, lm.sha256_rows(data, rows))
    pack, st = fs.pack(late)
    assert (st.spans, st.chunks, st.external_spans, st.chunk_bytes, st.pack_bytes, st.file_size) == \
        (len(rows), x.n_chunks, 0, LATE_N, x.layout["total"], LATE_N)
    assert pack.numel() == x.layout["total"]
    assert_index(torch, pack, x, "pack of late")
    assert lm.pack_data_mismatch(pack[x.layout["data"]:], torch.from_numpy(data).to(DEV), rows, x.chunk_span,
                                 x.chunk_off) is None
    got = to.unpack("late", pack, hasher=src["ch"])
    assert (got.spans, got.chunks, got.chunks_new, got.file_size) == (len(rows), x.n_chunks, x.n_chunks, LATE_N)
    h = to.open_file_readonly("late")
    g = Guard(LATE_N, 9)
    g.check(to.read_complete_device(h, g.ptr, LATE_N), data, "late, unpacked")


# ---- D. the delta ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def files(big, src, dst):
    """`src` alone: the receiving layer and its pack are released first."""
    import torch
    dst.clear()
    release(torch)
    fs = src["fs"]
    assert fs.verify_device(src["filler"], big.buf.data_ptr(), N_BIG) == (True, None)
    return src


def clone_of(files, name):
    fs = files["fs"]
    assert fs.clone_file("filler", name) == fs.stat(files["filler"])["spans"]
    return fs.open_file(name, files["ch"])


def assert_stats(r, ops, size_a, size_b, regions):
    lit = lm.delta_literal(ops)
    assert (r.n_ops, r.bytes_copy, r.bytes_literal, r.regions, r.size_a, r.size_b) == \
        (len(ops), size_b - lit, lit, regions, size_a, size_b), r
    assert r.bytes_literal <= r.bytes_literal_tables and r.seconds > 0


def test_delta_of_an_insert_past_the_line(big, files):
    import torch
    fs, a, host = files["fs"], files["filler"], big.host
    p, k = LINE + 99, 7
    ins = np.arange(k, dtype=np.uint8) + 201
    ins[0], ins[-1] = host[p] ^ 0x55, host[p - 1] ^ 0x55
    assert ins[0] != host[p] and ins[-1] != host[p - 1]                  # so neither search enters the insert
    b = clone_of(files, "ins")
    s = fs.insert(b, p, ins)
    assert (s.size_before, s.size_after) == (N_BIG, N_BIG + k)
    n_b = fs.stat(b)["spans"]
    t0 = time.perf_counter()
    r = fs.delta(a, b, literals=True)
    t0 = lap("delta", t0)
    want = lm.delta_insert(N_BIG, p, k)
    assert ops_of(r) == want == [(0, p, 0), (p, k, LIT), (p + k, N_BIG - p, p)]
    assert_stats(r, want, N_BIG, N_BIG + k, 1)
    assert k <= r.bytes_literal_tables <= REALIGN and n_b - REALIGN // S_STORE[0] <= r.spans_matched < n_b
    assert np.array_equal(r.literals.cpu().numpy(), ins)
    rebuilt = fs.apply_delta(a, r.ops, r.literals)
    t0 = lap("apply_delta", t0)
    assert rebuilt.numel() == N_BIG + k
    assert same_bytes(torch, rebuilt[:p], big.buf[:p]) and same_bytes(torch, rebuilt[p + k:], big.buf[p:])
    assert np.array_equal(rebuilt[p - 3:p + k + 3].cpu().numpy(), np.concatenate([host[p - 3:p], ins, host[p:p + 3]]))
    back = torch.full((N_BIG + k,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    assert fs.read_complete_device(b, back.data_ptr(), N_BIG + k) == N_BIG + k
    torch.cuda.synchronize()
    mem(torch)
    assert same_bytes(torch, rebuilt, back)
    mem(torch)
    t0 = lap("the comparisons", t0)
    del rebuilt, back
    release(torch)
    t = fs.delta(a, b, tables_only=True)
    ops = ops_of(t)
    assert [o for o, _, _ in ops] == [0] + np.cumsum([ln for _, ln, _ in ops])[:-1].tolist()
    assert sum(ln for _, ln, _ in ops) == N_BIG + k and t.bytes_literal == t.bytes_literal_tables == r.bytes_literal_tables
    (lo, ln, _), = [o for o in ops if o[2] == LIT]
    assert lo <= p and p + k <= lo + ln and ln <= REALIGN
    assert ops == [(0, lo, 0), (lo, ln, LIT), (lo + ln, N_BIG + k - lo - ln, lo + ln - k)]
    fs.remove_file("ins")


def test_delta_of_a_dropped_head_and_back(big, files):
    import torch
    fs, a, host = files["fs"], files["filler"], big.host
    d = LINE + 5
    size_b = N_BIG - d
    e = lm.common_prefix(host[d:], host)
    assert e < 8                                                         # measured; the closed forms take any
    b = clone_of(files, "tail")
    s = fs.delete_range(b, 0, d)
    assert (s.size_before, s.size_after) == (N_BIG, size_b) and fs.stat(b)["size"] == size_b
    g = Guard(size_b, 3)
    g.check(fs.read_complete_device(b, g.ptr, size_b), host[d:], "the file without its head")
    t0 = time.perf_counter()
    r = fs.delta(a, b)
    t0 = lap("delta A -> B, COPYs from past 2^32", t0)
    want = lm.delta_drop_head(N_BIG, d, e)
    assert ops_of(r) == want and want[-1] == (e, size_b - e, d + e) and d + e >= LINE
    assert_stats(r, want, N_BIG, size_b, 1)
    assert 0 < r.bytes_literal_tables <= REALIGN

    # the reverse: one LITERAL longer than 2^32 bytes, then a COPY on a diagonal below -2^32
    max_blocks = lm.csrc_const("kDlMaxBlocks", "delta.hip")
    assert max_blocks == 1 << 18
    r = fs.delta(b, a)
    lap("delta B -> A, the long LITERAL", t0)
    want = lm.delta_restore_head(N_BIG, d, e)
    assert ops_of(r) == want and want[-2:] == [(e, d - e, LIT), (d, N_BIG - d, 0)]
    assert_stats(r, want, size_b, N_BIG, 1)
    assert r.bytes_literal == d - e > LINE
    # the region the tables gave is A's spans up to the cut at which the two tables realign: every span that
    # begins below d holds bytes B lacks, so it is at least d - max long; its tiles outnumber the edge pass's blocks
    assert d - S_STORE[2] <= r.bytes_literal_tables <= d + REALIGN
    assert lm.delta_tiles(r.bytes_literal_tables) >= lm.delta_tiles(d - S_STORE[2]) > max_blocks
    mem(torch)
    fs.remove_file("tail")


def test_delta_with_a_slot_at_two_offsets_more_than_4_gib_apart(big, files):
    fs, host = files["fs"], big.host
    whole = big.chunks("fast", S_STORE)[1]
    head = oracle.fastcdc(host[:MIB], *S_STORE)
    assert np.array_equal(head[:3], whole[:3])                           # the first chunks of the stream, again
    b = clone_of(files, "dup")
    assert fs.write_to_file(b, big.buf[:MIB]) == len(head)               # appended: offsets N_BIG + ...
    size = N_BIG + MIB
    st = fs.stat(b)
    assert (st["size"], st["spans"]) == (size, len(whole) + len(head))
    slots, _ = slots_of(fs, b)
    offs = np.concatenate([whole[:, 0], head[:, 0] + np.uint64(N_BIG)])
    twice = [i for i in range(3) if slots[len(whole) + i] == slots[i]]
    assert twice and all(int(offs[i]) < MIB and int(offs[len(whole) + i]) >= N_BIG for i in twice)
    t0 = time.perf_counter()
    r = fs.delta(b, b)
    lap("delta of the file with itself", t0)
    want = lm.delta_self(size)
    assert ops_of(r) == want == [(0, size, 0)]
    assert_stats(r, want, size, size, 0)
    assert r.spans_matched == st["spans"] and r.bytes_literal_tables == 0
    fs.remove_file("dup")


def test_delta_of_a_truncation_to_the_line_and_back(big, files):
    fs, a, host = files["fs"], files["filler"], big.host
    t = LINE + 1
    b = clone_of(files, "cut")
    s = fs.truncate(b, t)
    assert (s.size_before, s.size_after) == (N_BIG, t)
    f = lm.common_suffix(host, host[:t])
    assert f < 8                                                         # measured; the closed form takes any
    whole = big.chunks("fast", S_STORE)[1]
    ragged = 0 if bool((whole[:, 0] == np.uint64(t)).any()) else 1       # the new end cuts a span short: one new slot
    r = fs.delta(a, b)
    want = lm.delta_truncate(N_BIG, t)
    assert ops_of(r) == want == [(0, t, 0)]
    assert_stats(r, want, N_BIG, t, ragged)
    r = fs.delta(b, a)
    want = lm.delta_extend(N_BIG, t, f)
    assert ops_of(r) == want and want[:2] == [(0, t, 0), (t, N_BIG - t - f, LIT)]
    assert_stats(r, want, t, N_BIG, 1)
    assert N_BIG - t <= r.bytes_literal_tables <= N_BIG - t + S_STORE[2]
    fs.remove_file("cut")
