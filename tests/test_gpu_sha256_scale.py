"""SHA-256 batches at the shapes the other tests never reach: the stream-table
paths of sha256_kernel and the longest-first claim order at scale.

Oracle: hashlib.sha256 per chunk, every comparison exact.  Chunk lists are
hand-made and go through sha256_batch_device, so no chunker is involved, and
every digest buffer is prefilled with 0xA5: a row the kernel never writes
(order[] not a permutation, a chunk claimed twice and another never) fails the
comparison instead of depending on what the allocation held before.

Branches of sha256.hip / Engine::sha256_batch these tests reach:

  * sha256_kernel<false, ...>, which reads first[] and the stream bases from
    global memory (more than kShaLdsStreams = 2048 streams): 5000 and 2049
    streams; the edge itself, 2048 streams with (2 * 2048 + 1) * 8 bytes of
    dynamic LDS, and 2047            -- test_stream_table_paths_one_handle
  * the regrowth of the stream table (sha_tab_cap_) and of the claim order
    (sha_order_cap_), and the rewriting of the pinned table by every call, on
    one handle: 3, 5000, 2048, 1, 2049, 2047 streams
                                      -- test_stream_table_paths_one_handle
  * the grid-stride loop of sha_hist_kernel (more than num_cus * 4 * 256
    chunks) and of sha_scatter_kernel (more than num_cus * 4 * 4096 chunks),
    the multi-tile cursor reservation and the 4095 / 4096 / 4097 tile edge
                                      -- test_claim_order_at_scale
  * len_class below 8 bytes (the oct < 3 branch) -- test_length_classes_below_8

The stream bases sit at every residue mod 4.  include/chunkfs_amd.h asks for
4-byte aligned bases; the kernel aligns the final address base + offset itself
(block_words), and these tests pin that it is indifferent to the base.

Out of scope:

  * Chunks of 512 MiB and more, whose bit length has a nonzero high word
    (W[14] = len >> 29).  One lane hashes a chunk sequentially, so such a test
    would run for tens of seconds; that path stays unverified.
  * Over-read detection.  The kernel reads 68-byte windows past a chunk's end
    when its successor in the same stream is contiguous and long enough; the
    bytes read past the end are masked out of the digest, so no digest can
    show an over-read across a stream edge (the `nhas` rule).  The adjacent
    streams whose offsets line up are here so that rule is at least exercised,
    and every stream lies at least 128 bytes inside the one allocation so
    nothing could fault; no data is placed at the end of an allocation.
"""
import hashlib

import numpy as np
import pytest

import store_model as sm

pytestmark = pytest.mark.gpu

FILL = 0xA5
MARGIN = 128          # every stream stays this far inside the allocation
MAX_STREAM = 700      # stream lengths 0..700
SHA_LDS_STREAMS = 2048  # sha256.hip kShaLdsStreams
SHA_TILE = 4096         # sha256.hip kShaTile


def _hash_rows(host, starts, chunks):
    """hashlib digests of chunks ((n, 2) offset/length) at host[start + offset ...], one start per chunk."""
    out = np.empty((len(chunks), 32), dtype=np.uint8)
    mv = memoryview(host)
    for i, ((o, ln), s) in enumerate(zip(chunks.tolist(), starts.tolist())):
        out[i] = np.frombuffer(hashlib.sha256(mv[s + o:s + o + ln]).digest(), dtype=np.uint8)
    return out


def _run(ch, ptrs, first, chunks):
    """sha256_batch_device into a digest buffer prefilled with FILL; returns the (n, 32) digests."""
    import torch
    n = int(first[-1])
    assert n == len(chunks)
    dc = sm.dev_chunks(chunks)
    dig = torch.full((max(n, 1), 32), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ch.sha256_batch_device(ptrs, first, dc.data_ptr(), dig.data_ptr())
    return dig[:n].cpu().numpy()


def _assert_per_stream(got, want, first, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        streams = np.unique(np.searchsorted(np.asarray(first, dtype=np.uint64), bad.astype(np.uint64), side="right") - 1)
        stale = int((got[bad] == FILL).all(axis=1).sum())
        raise AssertionError(f"{what}: {bad.size} wrong digests ({stale} never written), first at chunk "
                             f"{int(bad[0])}, streams {streams[:8].tolist()}")


def stream_layout(n_streams, seed):
    """Streams laid out back to back from MARGIN on, and their chunk lists.

    Returns (starts, lens, first, chunks, counts): start and length of every
    stream in the buffer, the first[] table, the (n, 2) chunk records with
    offsets relative to their stream, and how often each case occurs:
    junctions inside a stream that are contiguous with a successor >= 68 bytes
    / contiguous with a shorter successor / a gap, and adjacent stream pairs
    where the second's first offset equals the first's last offset + length.
    """
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, MAX_STREAM + 1, n_streams)
    empty = rng.random(n_streams) < 0.2
    if n_streams >= 8:      # runs of empty streams at the very start and the very end of the table
        empty[:3] = True
        empty[-3:] = True
        empty[3] = empty[-4] = False
    elif n_streams >= 3:
        empty[:] = False
        empty[0] = empty[-1] = True
    else:
        empty[:] = False
    lens[empty] = 0
    starts = np.zeros(n_streams, dtype=np.int64)
    at = MARGIN
    for i in range(n_streams):
        at += (int(rng.integers(0, 4)) - at) % 4  # the stream's base at a residue mod 4 of its own
        starts[i] = at
        at += int(lens[i])
    chunks, first = [], [0]
    counts = {"long_successor": 0, "short_successor": 0, "gap": 0, "edge_pairs": 0}
    prev_end = None  # offset + length of the previous stream's last chunk, if that stream is the one before
    for i in range(n_streams):
        L = int(lens[i])
        if L == 0:
            prev_end = None
            first.append(len(chunks))
            continue
        k = int(rng.integers(1, 5))
        pin = prev_end is not None and prev_end <= L and i % 2 == 0
        lo = prev_end if pin else int(rng.integers(0, max(L // 4, 1)))
        cuts = [lo] + sorted(int(c) for c in rng.integers(lo, L + 1, k))
        mine = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            ln = b - a
            if mine and ln and rng.random() < 0.34:  # a gap before this chunk: it starts later
                g = int(rng.integers(1, min(ln, 5) + 1))
                a, ln = a + g, ln - g
            mine.append((a, ln))
        for (a0, l0), (a1, l1) in zip(mine[:-1], mine[1:]):
            if a1 != a0 + l0:
                counts["gap"] += 1
            elif l1 >= 68:
                counts["long_successor"] += 1
            else:
                counts["short_successor"] += 1
        counts["edge_pairs"] += bool(pin)
        assert all(0 <= a and a + ln <= L for a, ln in mine)
        chunks.extend(mine)
        prev_end = mine[-1][0] + mine[-1][1]
        first.append(len(chunks))
    chunks = np.array(chunks, dtype=np.uint64).reshape(-1, 2)
    return starts, lens, np.array(first, dtype=np.uint64), chunks, counts


STREAM_COUNTS = [3, 5000, 2048, 1, 2049, 2047]
BUF_BYTES = MARGIN + max(STREAM_COUNTS) * (MAX_STREAM + 4) + MARGIN + 256


def test_stream_table_paths_one_handle():
    """One FastChunker handle hashes batches of 3, 5000, 2048, 1, 2049 and 2047
    streams, in that order: sha256_kernel<false> (5000, 2049: first[] and the
    bases read from global memory), the kShaLdsStreams edge (2048 streams with
    the largest LDS table, 2047, 2049), and small -> huge -> small on one handle
    (sha_tab_cap_ / sha_order_cap_ regrow once and are then reused by smaller
    batches; the pinned stream table is rewritten by every call).  Streams are
    slices of one buffer with bases at every residue mod 4; a fifth are empty,
    with runs of empty streams opening and closing the table (the binary
    search of first[] must skip them); chunks are contiguous with a long
    successor, contiguous with a short one, or behind a gap; some stream pairs
    have the second stream's first offset equal to the first's last offset +
    length (the `nhas` stream-edge rule, see the module docstring)."""
    import torch
    import chunkfs_amd as c
    host = np.random.default_rng(2024).integers(0, 256, BUF_BYTES, dtype=np.uint8)
    buf = sm.dev(host)
    assert buf.data_ptr() % 4 == 0
    ch = c.FastChunker(c.SizeParams(4096, 8192, 16384))
    assert min(STREAM_COUNTS[1], STREAM_COUNTS[4]) > SHA_LDS_STREAMS >= STREAM_COUNTS[2]
    for n_streams in STREAM_COUNTS:
        starts, lens, first, chunks, counts = stream_layout(n_streams, 1000 + n_streams)
        n = len(chunks)
        assert 0 < n <= 15000
        assert int(starts.min()) >= MARGIN and int((starts + lens).max()) + MARGIN <= host.size
        if n_streams >= 2047:
            assert {int(s) % 4 for s in starts} == {0, 1, 2, 3}
            assert 0.1 < float((lens == 0).mean()) < 0.3
            assert all(v > 20 for v in counts.values()), counts
        per_chunk_start = np.repeat(starts, np.diff(first.astype(np.int64)))
        want = _hash_rows(host, per_chunk_start, chunks)
        got = _run(ch, [buf.data_ptr() + int(s) for s in starts], first, chunks)
        _assert_per_stream(got, want, first, f"{n_streams} streams")
    del buf
    torch.cuda.synchronize()


# ---- the claim order at scale: a pooled oracle ----------------------------------
POOL_BYTES = 1 << 20


def make_pool(seed=77):
    """About 4096 distinct (offset, length) pairs over a POOL_BYTES buffer,
    offsets at every residue mod 4: every length 0..130, 2^k - 1 / 2^k / 2^k + 1
    up to 4096, two chunks of 64 KiB, and a spread of other lengths <= 300."""
    rng = np.random.default_rng(seed)
    lens = list(range(0, 131))
    for k in range(0, 13):
        lens += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    lens += [65536, 65536]
    lens = np.array(lens + rng.integers(0, 301, 4096 - len(lens)).tolist(), dtype=np.int64)
    offs = rng.integers(MARGIN, POOL_BYTES - 65536 - MARGIN - 4, lens.size)
    offs = offs - offs % 4 + np.arange(lens.size) % 4
    pool = np.unique(np.stack([offs, lens], axis=1), axis=0)
    pool = pool[rng.permutation(len(pool))].astype(np.uint64)
    assert int(pool[:, 0].min()) >= MARGIN and int((pool[:, 0] + pool[:, 1]).max()) + MARGIN <= POOL_BYTES
    return pool


@pytest.fixture(scope="module")
def pool():
    """(host bytes, device bytes, pool records, their hashlib digests), hashed once."""
    host = np.random.default_rng(4242).integers(0, 256, POOL_BYTES, dtype=np.uint8)
    recs = make_pool()
    dig = _hash_rows(host, np.zeros(len(recs), dtype=np.int64), recs)
    dig.setflags(write=False)
    recs.setflags(write=False)
    return host, sm.dev(host), recs, dig


@pytest.fixture(scope="module")
def scale_handle():
    import chunkfs_amd as c
    return c.FastChunker(c.SizeParams(4096, 8192, 16384))


def scale_counts(cus):
    """Chunk counts of test_claim_order_at_scale and the grids launch_sha256 gives them."""
    counts = {"tile-1": SHA_TILE - 1, "tile": SHA_TILE, "tile+1": SHA_TILE + 1,
              "hist-loop": cus * 4 * 256 + 1, "scatter-loop": cus * 4 * SHA_TILE + SHA_TILE + 77}
    grids = {}
    for k, n in counts.items():  # sha256.hip launch_sha256: sgrid, tgrid
        grids[k] = (min((n + 255) // 256, cus * 4), min((n + SHA_TILE - 1) // SHA_TILE, cus * 4))
    return counts, grids


@pytest.mark.parametrize("case", ["tile-1", "tile", "tile+1", "hist-loop", "scatter-loop"])
def test_claim_order_at_scale(pool, scale_handle, case):
    """The longest-first claim order (sha_hist_kernel, sha_scan_kernel,
    sha_scatter_kernel) must be a permutation at every size: 4095 / 4096 /
    4097 chunks (one scatter tile, exactly; a second tile of one chunk, so two
    blocks reserve runs from `cursor`), num_cus * 4 * 256 + 1 chunks (the
    grid-stride loop of sha_hist_kernel iterates) and num_cus * 4 * 4096 +
    4096 + 77 chunks (the grid-stride loop of sha_scatter_kernel iterates,
    with a ragged last tile).  A batch is pool[idx] for a random idx and the
    expected digests are pool_digests[idx]; a chunk the order misses keeps its
    0xA5 row, and one hashed from the wrong record gets another pool entry's
    digest.  The largest case is cut into three streams with one base pointer
    at arbitrary chunk indices."""
    import torch
    host, buf, recs, pool_dig = pool
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    counts, grids = scale_counts(cus)
    n = counts[case]
    print(f"{cus} CUs, {n} chunks, hist grid {grids[case][0]}, scatter grid {grids[case][1]}")
    # the loops iterate only where the chunk count exceeds what one pass of the capped grid covers
    assert counts["hist-loop"] > grids["hist-loop"][0] * 256 and grids["hist-loop"][0] == cus * 4
    assert counts["scatter-loop"] > grids["scatter-loop"][1] * SHA_TILE and grids["scatter-loop"][1] == cus * 4
    assert counts["scatter-loop"] > grids["scatter-loop"][0] * 256
    rng = np.random.default_rng(n)
    idx = rng.integers(0, len(recs), n)
    chunks = recs[idx]
    want = pool_dig[idx]
    sample = rng.integers(0, n, 48)  # the gathered oracle against hashlib, directly
    assert (want[sample] == _hash_rows(host, np.zeros(48, dtype=np.int64), chunks[sample])).all()
    if case == "scatter-loop":
        first = np.array([0, n // 3 + 1001, n - SHA_TILE - 5, n], dtype=np.uint64)
    else:
        first = np.array([0, n], dtype=np.uint64)
    got = _run(scale_handle, [buf.data_ptr()] * (len(first) - 1), first, chunks)
    _assert_per_stream(got, want, first, f"{n} chunks")


def test_length_classes_below_8(pool, scale_handle):
    """len_class for chunks shorter than 8 bytes (the oct < 3 branch, classes
    0..23): 64 chunks of lengths 0..7 only, shuffled, at every offset residue."""
    host, buf, _, _ = pool
    rng = np.random.default_rng(8)
    lens = rng.permutation(np.repeat(np.arange(8), 8))
    offs = MARGIN + 12 * np.arange(64) + np.arange(64) % 4
    chunks = np.stack([offs, lens], axis=1).astype(np.uint64)
    assert sorted(set(lens.tolist())) == list(range(8)) and {int(o) % 4 for o in offs} == {0, 1, 2, 3}
    first = np.array([0, 64], dtype=np.uint64)
    want = _hash_rows(host, np.zeros(64, dtype=np.int64), chunks)
    got = _run(scale_handle, [buf.data_ptr()], first, chunks)
    _assert_per_stream(got, want, first, "lengths 0..7")
