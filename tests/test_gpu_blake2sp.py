"""GPU suite of the BLAKE2sp kernel (chunkfs_amd/csrc/blake2sp.hip) through
cdc_hash_batch_device, against the hashlib oracle of tests/blake2sp_model.py.
Every digest row is prefilled with 0xA5 and compared whole.

What the cases reach in blake2sp.hip:

  * every chunk length 0..1100 at each start residue mod 4: empty leaves (all 8
    below 1 byte, some below 449), the 63/64/65 and 511/512/513 edges, a leaf
    that ends exactly on a block, the partial block on each of the 8 leaves,
    chunks of one, two and three steps, the guarded dword loads (gaps between
    the chunks: no contiguous successor) and the tail mask;
  * 4095..4097, 16383, 16384 and one 16 MiB chunk beside 63 short ones, all
    contiguous: the 16-byte loads past a chunk's end into its successor, the
    longest-first claim order, groups of one wave that leave at very different
    steps, the per-lane counter at 2 MiB;
  * streams that end on their buffer's last byte at each start and end residue;
  * 3, 2048 and 2049 streams with empty ones on one handle: the stream table in
    LDS, its largest size, and the table read from global memory;
  * 4095 / 4096 / 4097 chunks: the claim order's tile edge;
  * FastCDC's own chunk lists of a random and an all-zero stream.
"""
import hashlib

import numpy as np
import pytest

import blake2sp_model as bm
import oracle
import store_model as sm
from test_gpu_sha256_scale import BUF_BYTES, MARGIN, stream_layout

pytestmark = pytest.mark.gpu
FILL = 0xA5
MB = 1 << 20


@pytest.fixture(scope="module")
def handle():
    import chunkfs_amd as c
    return c.FastChunker(c.SizeParams(4096, 8192, 16384))


def _run(ch, ptrs, first, chunks, hash="blake2sp"):  # noqa: A002
    """hash_batch_device into digest rows prefilled with FILL; the (n, 32) digests."""
    import torch
    n = int(first[-1])
    assert n == len(chunks)
    dc = sm.dev_chunks(np.asarray(chunks, dtype=np.uint64).reshape(-1, 2) if n else np.zeros((1, 2), np.uint64))
    dig = torch.full((n + 1, 32), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ch.hash_batch_device(ptrs, first, dc.data_ptr(), dig.data_ptr(), hash=hash)
    out = dig.cpu().numpy()
    assert (out[n] == FILL).all(), "a digest was written past the last chunk's row"
    return out[:n]


def _want(host, chunks, starts=None):
    mv = host.tobytes()
    out = np.empty((len(chunks), 32), dtype=np.uint8)
    for i, (o, ln) in enumerate(np.asarray(chunks).tolist()):
        s = int(starts[i]) if starts is not None else 0
        out[i] = np.frombuffer(bm.oracle(mv[s + o:s + o + ln]), dtype=np.uint8)
    return out


def _assert_rows(got, want, chunks, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        stale = int((got[bad] == FILL).all(axis=1).sum())
        rows = [(int(i), [int(x) for x in np.asarray(chunks)[i]]) for i in bad[:8]]
        raise AssertionError(f"{what}: {bad.size} of {len(want)} digests wrong ({stale} never written); "
                             f"first (index, [offset, length]): {rows}")


def test_every_length_to_1100_at_every_alignment(handle):
    chunks, at = [], 64
    for a in range(4):
        for n in range(1101):
            at += (a - at) % 4
            chunks.append((at, n))
            at += n
    chunks = np.array(chunks, dtype=np.uint64)
    assert {(int(o) % 4, int(n)) for o, n in chunks} == {(a, n) for a in range(4) for n in range(1101)}
    host = np.random.default_rng(1).integers(0, 256, at + 64, dtype=np.uint8)
    buf = sm.dev(host)
    got = _run(handle, [buf.data_ptr()], [0, len(chunks)], chunks)
    _assert_rows(got, _want(host, chunks), chunks, "lengths 0..1100")


def test_long_chunks_and_one_16_mib_chunk_beside_63_short_ones(handle):
    rng = np.random.default_rng(2)
    lens = [4095, 4096, 4097, 16383, 16384] + rng.integers(0, 700, 31).tolist() + [16 * MB] + \
        rng.integers(0, 700, 32).tolist()
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    chunks = np.stack([offs, lens], axis=1).astype(np.uint64)  # contiguous: a start at every residue
    assert len(chunks) == 5 + 64
    host = rng.integers(0, 256, int(sum(lens)), dtype=np.uint8)
    buf = sm.dev(host)
    got = _run(handle, [buf.data_ptr()], [0, len(chunks)], chunks)
    _assert_rows(got, _want(host, chunks), chunks, "long chunks")


def test_streams_that_end_on_the_last_byte_of_their_buffer(handle):
    """16 streams, each a tensor of its own: the start of the first chunk at each
    residue mod 4, the buffer's length at each residue, the last chunk up to the
    last byte; and streams that are one chunk to the last byte."""
    rng = np.random.default_rng(3)
    hosts, bufs, chunks, first, starts = [], [], [], [0], []
    for a in range(4):
        for e in range(4):
            size = 1500 + 64 * a + e
            host = rng.integers(0, 256, size, dtype=np.uint8)
            mid = a + 300 + 7 * e
            mine = [(a, mid - a), (mid, size - mid)] if (a + e) % 2 else [(a, size - a)]
            hosts.append(host)
            bufs.append(sm.dev(host))
            chunks += mine
            starts += [len(hosts) - 1] * len(mine)
            first.append(len(chunks))
    chunks = np.array(chunks, dtype=np.uint64)
    got = _run(handle, [b.data_ptr() for b in bufs], first, chunks)
    want = np.stack([np.frombuffer(bm.oracle(hosts[s][int(o):int(o) + int(n)].tobytes()), dtype=np.uint8)
                     for s, (o, n) in zip(starts, chunks.tolist())])
    for s in range(len(hosts)):  # every stream's last chunk ends on its buffer's last byte
        o, n = chunks[first[s + 1] - 1].tolist()
        assert o + n == hosts[s].size and bufs[s].numel() == hosts[s].size
    _assert_rows(got, want, chunks, "last byte")


def test_3_2048_and_2049_streams_on_one_handle(handle):
    host = np.random.default_rng(2024).integers(0, 256, BUF_BYTES, dtype=np.uint8)
    buf = sm.dev(host)
    for n_streams in (3, 2048, 2049):
        starts, lens, first, chunks, _ = stream_layout(n_streams, 1000 + n_streams)
        assert int(starts.min()) >= MARGIN and int((starts + lens).max()) + MARGIN <= host.size
        assert (lens == 0).any()
        per_chunk_start = np.repeat(starts, np.diff(first.astype(np.int64)))
        got = _run(handle, [buf.data_ptr() + int(s) for s in starts], first, chunks)
        _assert_rows(got, _want(host, chunks, per_chunk_start), chunks, f"{n_streams} streams")


@pytest.fixture(scope="module")
def pool():
    """4097 chunk records over 256 KiB, hashed once: lengths 0..600 at every residue."""
    rng = np.random.default_rng(5)
    host = rng.integers(0, 256, 256 << 10, dtype=np.uint8)
    lens = rng.integers(0, 601, 4097)
    offs = rng.integers(64, host.size - 700, 4097)
    recs = np.stack([offs, lens], axis=1).astype(np.uint64)
    want = _want(host, recs)
    want.setflags(write=False)
    return host, sm.dev(host), recs, want


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_claim_order_tile_edge(handle, pool, n):
    host, buf, recs, want = pool
    got = _run(handle, [buf.data_ptr()], [0, n], recs[:n])
    _assert_rows(got, want[:n], recs[:n], f"{n} chunks")


@pytest.mark.parametrize("kind", ["random", "zero"])
def test_fastcdc_chunk_lists(handle, kind):
    host = np.random.default_rng(6).integers(0, 256, 4 * MB, dtype=np.uint8) if kind == "random" else \
        np.zeros(4 * MB, dtype=np.uint8)
    chunks = oracle.fastcdc(host, 4096, 8192, 16384)
    assert int(chunks[:, 1].sum()) == host.size and len(chunks) >= 256
    buf = sm.dev(host)
    got = _run(handle, [buf.data_ptr()], [0, len(chunks)], chunks)
    _assert_rows(got, _want(host, chunks), chunks, kind)


def test_sha256_through_the_new_call_equals_the_old_call(handle):
    import torch
    host = np.random.default_rng(7).integers(0, 256, MB, dtype=np.uint8)
    chunks = oracle.fastcdc(host, 4096, 8192, 16384)
    buf = sm.dev(host)
    n = len(chunks)
    got = _run(handle, [buf.data_ptr()], [0, n], chunks, hash="sha256")
    dc = sm.dev_chunks(chunks)
    old = torch.full((n, 32), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    handle.sha256_batch_device([buf.data_ptr()], [0, n], dc.data_ptr(), old.data_ptr())
    assert (got == old.cpu().numpy()).all()
    assert bytes(got[0]) == hashlib.sha256(host[:int(chunks[0, 1])].tobytes()).digest()
    assert handle.last_timing()["hash_ms"] > 0


def test_refusals_and_the_empty_batch(handle):
    import chunkfs_amd as c
    buf = sm.dev(np.zeros(64, dtype=np.uint8))
    dc = sm.dev_chunks(np.array([[0, 8]], dtype=np.uint64))
    dig = sm.dev(np.full(32, FILL, dtype=np.uint8))
    for args, words in ((([buf.data_ptr()], [1, 2]), "first[0] must be 0"),
                        (([buf.data_ptr(), buf.data_ptr()], [0, 2, 1]), "non-decreasing"),
                        (([0], [0, 1]), "NULL stream with chunks")):
        with pytest.raises(c.CdcError) as e:
            handle.hash_batch_device(*args, dc.data_ptr(), dig.data_ptr(), hash="blake2sp")
        assert e.value.code == c._lib.CDC_EINVAL and "cdc_hash_batch_device" in str(e.value) and words in str(e.value)
    with pytest.raises(c.CdcError) as e:
        handle.hash_batch_device([buf.data_ptr()], [0, 1], dc.data_ptr(), dig.data_ptr(), hash=7)
    assert e.value.code == c._lib.CDC_EINVAL and "unknown hasher 7" in str(e.value)
    handle.hash_batch_device([buf.data_ptr()], [0, 0], dc.data_ptr(), dig.data_ptr(), hash="blake2sp")
    assert (dig.cpu().numpy() == FILL).all()
    assert handle.last_timing()["hash_ms"] == 0
