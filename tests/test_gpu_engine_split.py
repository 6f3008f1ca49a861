"""The seams between the handle (Engine) and its backends (-m gpu): the
fixed-size path on its own buffers, cdc_last_timing across backends, the
hashers' scratch (HashEngine) across hashers and regrowth, the small
kernel's hand-over to the pipeline, and the host path (HostPath) on its own
buffers.  Every chunk list, every first[] and every
digest is compared bit for bit with the CPU oracle (no tolerances).
"""
import hashlib

import numpy as np
import pytest

import fast_sizes as fs
import oracle

pytestmark = pytest.mark.gpu

MIB = 1 << 20
PATH_PIPELINE, PATH_SMALL, PATH_WALK, PATH_FIXED, PATH_EMPTY = 0, 1, 2, 3, 4
FAST = (4096, 8192, 16384)


def _rows(out, first, n):
    rows = out[:int(first[n])].cpu().numpy().view(np.uint64).reshape(-1, 2)
    return [rows[int(first[i]):int(first[i + 1])] for i in range(n)]


def _same(got, want, what):
    assert got.shape == want.shape and (got == want).all(), what


# ---- 1. the fixed-size handle's own tables ----------------------------------------

FIXED_BIG = 9 * MIB  # one stream of this length: the batch exceeds 8 MiB and uploads its tables


def _fixed_script():
    """(name, [(offset, length)]) in call order: stream counts 1, 3, 64, 65
    (past the 64 streams that read the pinned tables in place; run twice, then
    with one length + 1 at the same pointers), 200 (regrows the 64-entry
    headroom), 3 again, an empty stream between two others, n = 0, and a batch
    with the 9 MiB stream (uploaded tables below 64 streams), twice."""
    rng = np.random.default_rng(11)

    def streams(k):
        lens = rng.integers(0, 300001, size=k)
        lens[rng.integers(0, k)] = 300000
        if k > 2:
            lens[rng.integers(0, k)] = 0
        return [(int(o), int(n)) for o, n in zip(rng.integers(0, FIXED_BIG - 300000, size=k), lens)]

    s65 = streams(65)
    s65_plus = list(s65)
    s65_plus[17] = (s65[17][0], s65[17][1] + 1)
    s3 = streams(3)
    big = [(0, FIXED_BIG), (4099, 300000), (7, 0), (123457, 1)]
    return [("1", streams(1)), ("3", s3), ("64", streams(64)), ("65", s65), ("65 again", s65),
            ("65, one length + 1", s65_plus), ("200", streams(200)), ("3 again", s3),
            ("empty between", [(5, 12345), (77, 0), (9, 4096)]), ("n = 0", []), ("9 MiB", big), ("9 MiB again", big),
            ("1 after all", [(3, 299999)])]


@pytest.mark.parametrize("cs", [4096, 1000])
def test_fixed_handle_on_its_own_buffers(cs):
    import torch
    import chunkfs_amd as c
    ch = c.FSChunker(cs)
    buf = torch.zeros(FIXED_BIG + 64, dtype=torch.uint8, device="cuda:0")
    for name, st in _fixed_script():
        lens = [n for _, n in st]
        cap = ch.batch_max_chunks(lens)
        out = torch.zeros((max(cap, 1), 2), dtype=torch.int64, device="cuda:0")
        first = ch.chunk_batch_device([buf.data_ptr() + o for o, _ in st], lens, out.data_ptr(), cap)
        want = [oracle.fixed(n, cs) if n else np.zeros((0, 2), np.uint64) for n in lens]
        want_first = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
        assert (np.asarray(first, dtype=np.uint64) == want_first).all(), (cs, name, first, want_first)
        for i, (g, w) in enumerate(zip(_rows(out, first, len(st)), want)):
            _same(g, w, (cs, name, "stream", i))
        t = ch.last_timing()
        assert t["path"] == (PATH_FIXED if st else PATH_EMPTY), (cs, name, t)
        assert t["bytes"] == sum(lens)
    data = np.zeros(300001, dtype=np.uint8)
    _same(ch.chunk_array(data), oracle.fixed(data.size, cs), (cs, "cdc_chunk_data"))
    assert ch.last_timing()["path"] == PATH_FIXED
    assert ch.batch_sync() == 0
    ch.close()


# ---- 2. cdc_last_timing across backends ---------------------------------------------

BATCH = 12 * MIB


def _device_batch(ch, torch, dev, off, n, sync=True):
    cap = ch.batch_max_chunks([n])
    out = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
    call = ch.chunk_batch_device if sync else ch.chunk_batch_device_async
    return out, call([dev.data_ptr() + off], [n], out.data_ptr(), cap)


def _hash_then_batch(ch, torch, cut, path):
    """cdc_chunk_and_hash on 1 MiB, then a 12 MiB synchronous device batch:
    hash_ms stays the hash call's, the rest of cdc_last_timing is the batch's."""
    small = oracle.splitmix64_bytes(MIB, 21)
    chunks, dig = ch.chunk_and_hash(small)
    _same(chunks, cut(small), "cdc_chunk_and_hash chunks")
    for (o, n), d in zip(chunks, dig):
        assert bytes(d) == hashlib.sha256(small[int(o):int(o + n)].tobytes()).digest()
    t0 = ch.last_timing()
    assert t0["hash_ms"] > 0 and t0["bytes"] == MIB
    data = oracle.splitmix64_bytes(BATCH + 5 * 4096, 22)
    dev = torch.from_numpy(data).to("cuda:0")
    out, first = _device_batch(ch, torch, dev, 0, BATCH)
    _same(_rows(out, first, 1)[0], cut(data[:BATCH]), "12 MiB synchronous batch")
    t = ch.last_timing()
    print(f"path {path}: hash call {t0}, batch {t}")
    assert t["hash_ms"] == t0["hash_ms"]
    assert t["path"] == path and t["bytes"] == BATCH and t["timed"] == 1 and t["total_ms"] > 0
    return data, dev, t


def test_timing_across_backends_fastcdc():
    """The hash_ms carry, then an async burst of 5 batches of 12 MiB read back
    with cdc_debug_timing_back(0..4) and no cdc_batch_sync in between: the
    forwarder drains them, `timed` is 1 exactly for the batches whose
    sequence number CHUNKFS_AMD_EVENT_EVERY (4) divides, and the cdc_batch_sync
    that follows returns the fifth batch's chunk count (held)."""
    import torch
    import chunkfs_amd as c
    cut = lambda a: oracle.fastcdc(a, *FAST)  # noqa: E731
    ch = c.FastChunker(c.SizeParams(*FAST))
    data, dev, t = _hash_then_batch(ch, torch, cut, PATH_PIPELINE)
    alone = c.FastChunker(c.SizeParams(*FAST))  # the same batch on a handle that ran nothing else
    _device_batch(alone, torch, dev, 0, BATCH)
    ta = alone.last_timing()
    alone.close()
    assert ta["hash_ms"] == 0
    assert (t["candidates"], t["overflow_spans"], t["fixup_iterations"]) == \
        (ta["candidates"], ta["overflow_spans"], ta["fixup_iterations"]) and t["candidates"] > 0
    # pipeline batches so far: the synchronous one, and one per small-kernel fallback
    base = 1 + c.host_stats(ch)["small_fallbacks"]
    burst = [_device_batch(ch, torch, dev, j * 4096, BATCH, sync=False) for j in range(5)]
    backs = [ch.timing_back(k) for k in range(5)]
    for k, tb in enumerate(backs):
        j = 4 - k
        assert tb["path"] == PATH_PIPELINE and tb["timed"] == (1 if (base + j) % 4 == 0 else 0), (k, base, tb)
        assert (tb["total_ms"] > 0) == bool(tb["timed"])
        assert tb["hash_ms"] == t["hash_ms"]
    want = [cut(data[j * 4096:j * 4096 + BATCH]) for j in range(5)]
    for j, (out, first) in enumerate(burst):
        assert int(first[0]) == 0 and int(first[1]) == len(want[j]), (j, first)
        _same(_rows(out, first, 1)[0], want[j], ("async batch", j))
    assert ch.batch_sync() == len(want[4])
    assert ch.batch_sync() == 0
    ch.close()


def test_timing_across_backends_rabin():
    import torch
    import chunkfs_amd as c
    ch = c.RabinChunker(c.SizeParams(*FAST))
    _hash_then_batch(ch, torch, lambda a: oracle.cdc("rabin", a, *FAST), PATH_WALK)
    ch.close()


def test_hash_scratch_across_hashers_and_regrowth():
    """The HashEngine's buffers on one handle, both hashers alternating: a first
    call that sizes them for 1 stream and 3 chunks (1 / 67 / 69 bytes from an odd
    address), 5000 chunks (the order buffer regrows; past the 4096-chunk scatter
    tile), 2049 streams (the stream table regrows and is read from global
    memory), a chunking batch in between that leaves hash_ms alone, and a last
    call smaller than everything allocated.  Every digest against the host's."""
    import torch
    import chunkfs_amd as c
    from test_gpu_blake2sp import _assert_rows, _run, _want
    from test_gpu_sha256 import _digests
    rng = np.random.default_rng(41)
    host = rng.integers(0, 256, MIB + 4096, dtype=np.uint8)
    dev = torch.from_numpy(host).to("cuda:0")
    ch = c.FastChunker(c.SizeParams(*FAST))

    # 1. SHA-256: the first chunk starts at byte 1 of the buffer
    recs = np.array([(1, 1), (2, 67), (69, 69)], dtype=np.uint64)
    got = _run(ch, [dev.data_ptr()], [0, 3], recs, hash="sha256")
    _assert_rows(got, _digests(host, recs), recs, "call 1, SHA-256, 3 chunks")
    assert ch.last_timing()["hash_ms"] > 0

    # 2. BLAKE2sp: 5000 chunks of 64..600 bytes
    recs = np.stack([rng.integers(64, MIB - 700, 5000), rng.integers(64, 601, 5000)], axis=1).astype(np.uint64)
    got = _run(ch, [dev.data_ptr()], [0, 5000], recs)
    _assert_rows(got, _want(host, recs), recs, "call 2, BLAKE2sp, 5000 chunks")

    # 3. SHA-256: 2049 streams (4-byte aligned) of one chunk each
    starts = 4 * rng.integers(0, (MIB - 700) // 4, 2049)
    recs = np.stack([rng.integers(0, 4, 2049), rng.integers(0, 601, 2049)], axis=1).astype(np.uint64)
    got = _run(ch, [dev.data_ptr() + int(s) for s in starts], list(range(2050)), recs, hash="sha256")
    absolute = np.stack([starts + recs[:, 0].astype(np.int64), recs[:, 1].astype(np.int64)], axis=1)
    _assert_rows(got, _digests(host, absolute), recs, "call 3, SHA-256, 2049 streams")
    t3 = ch.last_timing()
    assert t3["hash_ms"] > 0

    # 4. a chunking batch reports its own timing and call 3's hash_ms
    out, first = _device_batch(ch, torch, dev, 0, MIB)
    _same(_rows(out, first, 1)[0], oracle.fastcdc(host[:MIB], *FAST), "call 4, 1 MiB batch")
    t4 = ch.last_timing()
    assert t4["bytes"] == MIB and t4["hash_ms"] == t3["hash_ms"], (t3, t4)

    # 5. BLAKE2sp: an empty chunk and one of 513 bytes
    recs = np.array([(5, 0), (7, 513)], dtype=np.uint64)
    got = _run(ch, [dev.data_ptr()], [0, 2], recs)
    _assert_rows(got, _want(host, recs), recs, "call 5, BLAKE2sp, 2 chunks")
    assert ch.last_timing()["hash_ms"] > 0
    ch.close()


# ---- 3. small kernel -> pipeline hand-over -------------------------------------------

def _counters(c, ch):
    st = c.host_stats(ch)
    return st["small_calls"], st["small_fallbacks"], st["guard_trips"]


def test_small_kernel_hand_over():
    """cdc_chunk_data where the model says the one-launch kernel is off (64 /
    256 / 1024: the masks have fewer than 10 bits), then on a 4 / 8 / 16 KiB
    handle 1 MiB of zeros and 1 MiB of random bytes, alternating eight times.

    The model (fast_sizes.small_eligible) says which calls the kernel is tried
    on: every one of the second handle.  It has no prediction for the
    fallbacks; the counts below are recorded, not derived: the parent commit
    of the FastEngine split gave, on these inputs, one small call and no
    fallback per call, zeros and random bytes alike (a zero run has one hash
    value, which the built-in table's masks reject: no record, max-size cuts)."""
    import chunkfs_amd as c
    p = fs.params(64, 256, 1024)
    data = oracle.splitmix64_bytes(MIB, 31)
    assert p.pmin < 10 and not fs.small_eligible(p, data.size)
    ch = c.FastChunker(c.SizeParams(64, 256, 1024))
    _same(ch.chunk_array(data), oracle.fastcdc(data, 64, 256, 1024), "64/256/1024")
    assert _counters(c, ch) == (0, 0, 0)
    ch.close()

    p = fs.params(*FAST)
    zeros = np.zeros(MIB, dtype=np.uint8)
    inputs = [("zeros", zeros, oracle.fastcdc(zeros, *FAST)), ("random", data, oracle.fastcdc(data, *FAST))]
    recorded_fallbacks = {"zeros": 0, "random": 0}
    ch = c.FastChunker(c.SizeParams(*FAST))
    calls = fallbacks = 0
    for rep in range(8):
        for name, a, want in inputs:
            _same(ch.chunk_array(a), want, (rep, name))
            calls += 1 if fs.small_eligible(p, a.size) else 0
            fallbacks += recorded_fallbacks[name]
            got = _counters(c, ch)
            print(f"rep {rep} {name}: small calls, fallbacks, guard trips {got}")
            assert got == (calls, fallbacks, 0), (rep, name)
    assert calls == 16
    ch.close()


# ---- 4. the host path on its own buffers --------------------------------------------

@pytest.mark.parametrize("sizes", [FAST, (64, 256, 1024)])
def test_host_path_on_its_own_buffers(sizes):
    """HostPath's buffers on one handle, every call in this order: a 64 KiB
    cdc_chunk_data that sizes everything small; a write of 5 MiB + 1 byte in
    1 MiB segments (one short), whose window regrows the host-mapped chunk list
    after cdc_chunk_data sized it and reads it through the same waiting,
    checking reader; cdc_chunk_and_hash of 1 MiB, then of 3 MiB (the chunk list
    in HBM and the digests regrow); 17 MiB (past the 16 MiB ring limit: the
    pageable copy, the data buffer regrows); 5 MiB (two ring pieces, 4 + 1 MiB);
    64 KiB again (every buffer larger than it needs); a last write of 1 MiB +
    17 bytes.  On 4 / 8 / 16 KiB the one-launch kernel takes the calls of up
    to 4 MiB; on 64 / 256 / 1024 it is off and the chunk counts are large, so
    every buffer regrows.  The guard never trips."""
    import chunkfs_amd as c
    cut = lambda a: oracle.fastcdc(a, *sizes)  # noqa: E731
    data = oracle.splitmix64_bytes(17 * MIB, 51)
    ch = c.FastChunker(c.SizeParams(*sizes))

    def chunked(n, step):
        _same(ch.chunk_array(data[:n]), cut(data[:n]), (sizes, step))
        assert c.host_stats(ch)["guard_trips"] == 0, (sizes, step)

    def written(a, step):
        spans, _ = c.write_spans(ch, a, seg_size=MIB)
        _same(spans, cut(a)[:, 1], (sizes, step))
        assert c.host_stats(ch)["guard_trips"] == 0, (sizes, step)

    def hashed(a, step):
        chunks, dig = ch.chunk_and_hash(a)
        _same(chunks, cut(a), (sizes, step))
        for (o, n), d in zip(chunks, dig):
            assert bytes(d) == hashlib.sha256(a[int(o):int(o + n)].tobytes()).digest(), (sizes, step, int(o))
        assert c.host_stats(ch)["guard_trips"] == 0, (sizes, step)

    chunked(64 << 10, "1: 64 KiB")
    written(oracle.splitmix64_bytes(5 * MIB + 1, 52), "2: write of 5 MiB + 1")
    hashed(oracle.splitmix64_bytes(MIB, 53), "3: hash 1 MiB")
    hashed(oracle.splitmix64_bytes(3 * MIB, 54), "3: hash 3 MiB")
    chunked(17 * MIB, "4: 17 MiB")
    chunked(5 * MIB, "5: 5 MiB")
    chunked(64 << 10, "6: 64 KiB again")
    written(oracle.splitmix64_bytes(MIB + 17, 55), "7: write of 1 MiB + 17")
    ch.close()
