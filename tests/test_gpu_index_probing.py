"""Dedup index probing, 64-bit key collisions and totals, with crafted digests.

Digests are the caller's (DedupIndex.insert_device, ChunkStore.put_device), so
these tests choose them to reach what real SHA-256 digests in a table a few
percent full never do.  From index.hip: key = little-endian u64 of digest bytes
0..7, | 1; home slot = (key >> 1) & (slots - 1); slots is a power of two (today
max(1024, pow2 >= 2 * capacity)).  `crafted` below is the one place that recipe
is written down.

The oracle throughout is a Python dict fed in chunk order, the first insert of
a digest winning (the reference's Database, src/system/database.rs:74-77);
every comparison is exact.

Branches reached:

  * the probe wrap `s = (s + 1) & mask` in claim_kernel (index.hip) and in the
    store's lookup_kernel (store.hip): clusters that start in the last slot(s)
    and continue at slot 0 -- test_wrap_around_cluster_index,
    test_wrap_around_cluster_store (found and never-stored digests),
    test_merged_clusters_straddle_the_table_end
  * the same wrap in serial_kernel, and `pending` filled by many waves of
    several blocks in arbitrary order, in-batch duplicates of colliding
    digests, collisions against entries an earlier batch's serial pass placed
    -- test_key_collisions_across_blocks_index / _store (their colliding group
    has its home in the last slot, so the serial pass's probe wraps at once)
  * mark_kernel's 64-bit reductions over partial waves, with totals far above
    2^32 -- test_partial_waves_and_64_bit_totals

Not tested: the kIndexPendingCap boundary (4096 queued collisions in one
batch) and its overflow error.  The serial pass is quadratic on one thread; at
4096 pending entries it would run for many seconds.  The colliding entries per
batch stay at or below about 400 here for the same reason.

Both the index and the store refuse a batch of n entries unless unique + n <=
capacity (every entry might be new).  A table created for 512 digests can
therefore take its last 256 only in a batch without duplicates; the wrap
tests run at capacity 512 that way (after checking that the batch with
duplicates is refused and changes nothing) and at capacity 1024 with
duplicates in every batch.
"""
import numpy as np
import pytest

import store_model as sm

pytestmark = pytest.mark.gpu

HOME_BITS = 20  # the recipe reaches tables of up to 2^20 slots


def crafted(j, home_delta, rng):
    """(len(j), 32) digests whose index key is (j << 21) | (home << 1) | 1 with
    home = home_delta mod 2^20 in key bits 1..20: the home slot is (slots +
    home_delta) mod slots for every table of up to 2^20 slots -- home_delta -1
    is the last slot whatever the table's size.  Bytes 8..31 are random."""
    j = np.asarray(j, dtype=np.uint64)
    home = (np.asarray(home_delta, dtype=np.int64) % (1 << HOME_BITS)).astype(np.uint64)
    assert int(j.max()) < 1 << (63 - HOME_BITS)
    key = (j << np.uint64(HOME_BITS + 1)) | (home << np.uint64(1)) | np.uint64(1)
    dig = rng.integers(0, 256, (j.size, 32), dtype=np.uint8)
    dig[:, :8] = key.astype("<u8").view(np.uint8).reshape(-1, 8)
    return dig


def keys_of(dig):
    """index.hip key_of, recomputed: LE u64 of bytes 0..7, | 1."""
    return np.ascontiguousarray(dig[:, :8]).view("<u8").reshape(-1) | np.uint64(1)


def homes_of(dig, slots):
    return (keys_of(dig) >> np.uint64(1)) & np.uint64(slots - 1)


def distinct_j(rng, n):
    j = np.unique(rng.integers(0, 1 << 40, 2 * n + 16))
    assert j.size >= n
    return rng.permutation(j)[:n]


def with_dups(rng, fresh, earlier, n_earlier, n_within):
    """`fresh` digests interleaved with n_within repeats of themselves and
    n_earlier repeats of `earlier` ones, shuffled."""
    parts = [fresh]
    if n_within:
        parts.append(fresh[rng.integers(0, len(fresh), n_within)])
    if n_earlier:
        parts.append(earlier[rng.integers(0, len(earlier), n_earlier)])
    batch = np.concatenate(parts)
    return batch[rng.permutation(len(batch))]


class DictIndex:
    """The oracle: digest -> length of its first insert, and the written totals."""

    def __init__(self):
        self.db, self.chunks_written, self.bytes_written = {}, 0, 0

    def insert(self, dig, lens):
        new = np.zeros(len(dig), dtype=np.uint8)
        for i, (d, ln) in enumerate(zip(dig, lens)):
            k = bytes(d)
            new[i] = k not in self.db
            self.db.setdefault(k, int(ln))
            self.chunks_written += 1
            self.bytes_written += int(ln)
        return new

    def stats(self):
        return {"chunks_written": self.chunks_written, "bytes_written": self.bytes_written,
                "unique_chunks": len(self.db), "unique_bytes": sum(self.db.values())}


def index_insert(ix, dig, lens):
    """insert_device of host digests / lengths; returns (count, u8 flags).  The
    index reads only the chunk records' lengths, never a data buffer."""
    import torch
    n = len(dig)
    chunks = np.stack([np.arange(n, dtype=np.uint64), np.asarray(lens, dtype=np.uint64)], axis=1)
    dd, dc = sm.dev(dig), sm.dev_chunks(chunks)
    new = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n_new = ix.insert_device(dd.data_ptr(), dc.data_ptr(), n, new.data_ptr())
    return n_new, new.cpu().numpy()


def insert_checked(ix, model, dig, lens):
    want = model.insert(dig, lens)
    n_new, new = index_insert(ix, dig, lens)
    assert (new == want).all(), f"new flags differ at {np.flatnonzero(new != want)[:8].tolist()}"
    assert n_new == int(want.sum())
    st, ws = ix.stats(), model.stats()
    for k, v in ws.items():
        assert st[k] == v, (k, st[k], v)
    if ws["unique_bytes"]:
        assert st["cdc_dedup_ratio"] == ws["bytes_written"] / ws["unique_bytes"]
    return want


def store_put_checked(st, model, d_data, data, chunks, dig):
    """put_device of crafted digests: the model keeps the first bytes a digest came with."""
    want = np.zeros(len(dig), dtype=bool)
    for i, ((o, ln), d) in enumerate(zip(chunks.tolist(), dig)):
        k = bytes(d)
        want[i] = k not in model.db
        model.db.setdefault(k, data[o:o + ln].tobytes())
        model.chunks_written += 1
        model.bytes_written += ln
    new = sm.put(st, d_data, data.size, chunks, dig)
    assert (new == want).all(), f"new flags differ at {np.flatnonzero(new != want)[:8].tolist()}"
    sm.assert_stats(st, model)
    return want


class Payloads:
    """Small distinct chunks of one random buffer: entry k of a test takes the
    next one, so a repeated digest arrives with other bytes than its first insert."""

    def __init__(self, seed, n):
        rng = np.random.default_rng(seed)
        self.data = rng.integers(0, 256, 64 * n + 64, dtype=np.uint8)
        self.lens = rng.integers(1, 49, n)
        self.at = 0

    def take(self, n):
        k = np.arange(self.at, self.at + n)
        self.at += n
        assert self.at <= len(self.lens)
        return np.stack([64 * k + k % 16, self.lens[k]], axis=1).astype(np.uint64)


# ---- 1. a cluster that starts in the last slot -----------------------------------
def wrap_batches(seed=21):
    """512 digests with distinct keys (j << 21) | 0x1FFFFF, all at home in the
    last slot, as three batches of 1, 255 and 256 new digests.  Returns (all
    512, [batch 1, batch 2, batch 3 with duplicates, batch 3 without], 50 more
    digests of the same home that no batch holds)."""
    rng = np.random.default_rng(seed)
    dig = crafted(distinct_j(rng, 562), -1, rng)
    dig, absent = dig[:512], dig[512:]
    a, b, c3 = dig[:1], dig[1:256], dig[256:]
    return dig, [with_dups(rng, a, a, 0, 2), with_dups(rng, b, a, 40, 90),
                 with_dups(rng, c3, dig[:256], 60, 60), c3[rng.permutation(256)]], absent


def _lens(rng, n):
    return rng.integers(0, 20000, n)


@pytest.mark.parametrize("capacity", [512, 1024])
def test_wrap_around_cluster_index(capacity):
    """claim_kernel's `s = (s + 1) & mask`: 512 distinct keys at home in the last
    slot form one cluster that wraps to slot 0 at its second entry and ends
    511 slots later; every later insert of the cluster probes across the
    table end.  Flags, count and stats after each batch, against the dict."""
    import chunkfs_amd as c
    dig, batches, _ = wrap_batches()
    rng = np.random.default_rng(capacity)
    ix, model = c.DedupIndex(capacity), DictIndex()
    insert_checked(ix, model, batches[0], _lens(rng, len(batches[0])))
    want = insert_checked(ix, model, batches[1], _lens(rng, len(batches[1])))
    assert 0 < int(want.sum()) < len(want)
    if capacity == 512:  # 256 unique + 376 entries > 512: refused before the table is touched
        before = ix.stats()
        with pytest.raises(c.CdcError) as ei:
            index_insert(ix, batches[2], _lens(rng, len(batches[2])))
        assert ei.value.code == c._lib.CDC_ENOMEM
        assert ix.stats() == before
        insert_checked(ix, model, batches[3], _lens(rng, 256))
    else:
        want = insert_checked(ix, model, batches[2], _lens(rng, len(batches[2])))
        assert 0 < int(want.sum()) < len(want)
    assert ix.stats()["unique_chunks"] == 512


@pytest.mark.parametrize("max_chunks", [512, 1024])
def test_wrap_around_cluster_store(max_chunks):
    """The same cluster through ChunkStore.put_device, then lookup_kernel's own
    copy of the probe loop: contains and get of all 512 digests in reversed
    order (each probe runs from the last slot across the table end to its
    entry), and 50 never-stored digests of the same home, which are absent only
    after a probe over the whole wrapped cluster to the first empty slot."""
    import torch
    import chunkfs_amd as c
    dig, batches, absent = wrap_batches()
    pay = Payloads(5, 1200)
    d_data = sm.dev(pay.data)
    st, model = c.ChunkStore(max_chunks, 1 << 17), sm.Model()
    for b in (batches[0], batches[1], batches[3] if max_chunks == 512 else batches[2]):
        store_put_checked(st, model, d_data, pay.data, pay.take(len(b)), b)
    assert st.stats()["unique_chunks"] == 512
    req = np.concatenate([dig[::-1], absent])
    dd = sm.dev(req)
    found = torch.full((len(req),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert st.contains_device(dd.data_ptr(), len(req), found.data_ptr()) == 512
    assert found.cpu().numpy().tolist() == [1] * 512 + [0] * 50
    sm.get_checked(st, model, dig[::-1])
    with pytest.raises(c.CdcError) as ei:
        st.get_device(dd.data_ptr(), len(req), None, 0)
    assert ei.value.code == c._lib.CDC_ENOTFOUND


# ---- 2. clusters that merge across the table end ----------------------------------
def merged_batches(seed=22):
    """600 digests at home in the 8 adjacent slots slots - 4 .. slots + 3 (mod
    slots), shuffled, as two batches of 300 new digests with duplicates."""
    rng = np.random.default_rng(seed)
    delta = rng.permutation(np.arange(600) % 8 - 4)
    dig = crafted(distinct_j(rng, 600), delta, rng)
    return dig, delta, [with_dups(rng, dig[:300], dig[:300], 0, 100), with_dups(rng, dig[300:], dig[:300], 120, 80)]


def test_merged_clusters_straddle_the_table_end():
    """Eight neighbouring homes on both sides of the table end: the clusters grow
    into each other, so a probe passes entries of other homes, crosses the
    wrap and goes on (claim_kernel).  Two batches into an index of capacity 1024."""
    import chunkfs_amd as c
    _, _, batches = merged_batches()
    rng = np.random.default_rng(2)
    ix, model = c.DedupIndex(1024), DictIndex()
    for b in batches:
        want = insert_checked(ix, model, b, _lens(rng, len(b)))
        assert 0 < int(want.sum()) < len(want)
    assert ix.stats()["unique_chunks"] == 600


# ---- 3. 64-bit key collisions across blocks -----------------------------------------
def collision_batches(seed=23):
    """350 digests sharing one 8-byte prefix (home: the last slot), among them
    pairs that differ only in bit 0 of byte 0 and pairs that differ only in
    byte 31; 300 unrelated digests.  Batch 1: the first 300 colliding, the
    unrelated ones and duplicates of both, 1000 entries shuffled (four
    256-thread blocks).  Batch 2: a shuffled subset of batch 1 plus the other
    50 colliding digests.  Returns (colliding, unrelated, [batch 1, batch 2])."""
    rng = np.random.default_rng(seed)
    base = crafted(np.full(117, 0x5EED5EED), -1, rng)  # one key; random bytes 8..31
    flip0 = base[:117].copy()
    flip0[:, 0] ^= 1            # the key forces bit 0: the same key
    flip31 = base[:116].copy()
    flip31[:, 31] ^= 0x80
    coll = np.concatenate([base, flip0, flip31])
    coll = coll[rng.permutation(350)]
    assert len({bytes(d) for d in coll}) == 350
    unrel = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    b1 = np.concatenate([coll[:300], unrel, coll[rng.integers(0, 300, 100)], unrel[rng.integers(0, 300, 300)]])
    b1 = b1[rng.permutation(len(b1))]
    b2 = np.concatenate([coll[rng.permutation(300)[:100]], unrel[rng.permutation(300)[:150]], coll[300:]])
    b2 = b2[rng.permutation(len(b2))]
    return coll, unrel, [b1, b2]


def test_key_collisions_across_blocks_index():
    """verify_kernel -> pending -> serial_kernel with about 400 colliding entries
    spread over four blocks: `pending` fills in whatever order the waves run,
    the serial pass takes it by chunk index, meets in-batch duplicates of
    colliding digests, and in the second batch finds the entries the first
    batch's serial pass placed and adds 50 more behind them.  The colliding
    key's home is the last slot, so serial_kernel's probe wraps at once.  The
    flags equal the dict's for every entry and are the same on a rerun against
    a fresh index: the order of `pending` does not reach the results."""
    import chunkfs_amd as c
    _, _, batches = collision_batches()
    flags = []
    for run in range(2):
        rng = np.random.default_rng(3)
        ix, model = c.DedupIndex(2048), DictIndex()
        got = []
        for b in batches:
            want = insert_checked(ix, model, b, _lens(rng, len(b)))
            assert 0 < int(want.sum()) < len(want)
            got.append(want)
        assert ix.stats()["unique_chunks"] == 650
        flags.append(np.concatenate(got))
    assert (flags[0] == flags[1]).all()


def test_key_collisions_across_blocks_store():
    """The same batches through ChunkStore put and get: every colliding digest
    gives back the bytes of its own first insert (lookup_kernel probes past tag
    matches of other digests, across the table end), repeats arrive with other
    bytes and change nothing."""
    import chunkfs_amd as c
    coll, unrel, batches = collision_batches()
    pay = Payloads(6, 1400)
    d_data = sm.dev(pay.data)
    st, model = c.ChunkStore(2048, 1 << 17), sm.Model()
    for b in batches:
        store_put_checked(st, model, d_data, pay.data, pay.take(len(b)), b)
    assert st.stats()["unique_chunks"] == 650
    every = np.concatenate([coll, unrel])
    sm.get_checked(st, model, every[np.random.default_rng(4).permutation(650)])


# ---- 4. partial waves and 64-bit totals -----------------------------------------------
TOTALS_BATCH_SIZES = [1, 63, 64, 65, 255, 257]


def totals_batches(seed=24):
    """Batches of TOTALS_BATCH_SIZES entries of random digests, a third of each
    repeats (of earlier batches and of the batch itself), with lengths around
    2^32, 2^40 + 3 and small values mixed.  Returns [(digests, lengths)]."""
    rng = np.random.default_rng(seed)
    big = np.array([2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3, 0, 1, 4096, 77777], dtype=np.uint64)
    seen, out = np.zeros((0, 32), dtype=np.uint8), []
    for n in TOTALS_BATCH_SIZES:
        n_dup = n // 3
        fresh = rng.integers(0, 256, (n - n_dup, 32), dtype=np.uint8)
        n_old = min(n_dup // 2, len(seen))
        b = with_dups(rng, fresh, seen, n_old, n_dup - n_old)
        assert len(b) == n
        out.append((b, big[rng.integers(0, len(big), n)]))
        seen = np.concatenate([seen, fresh])
    return out


def test_partial_waves_and_64_bit_totals():
    """mark_kernel's __shfl_xor reductions of bytes written / unique bytes /
    unique chunks: batches of 1, 63, 64, 65, 255 and 257 entries (a lone lane,
    a wave short of one lane, one full wave, a wave plus one lane, a block
    short of one lane, a block plus one lane) with lengths of 2^32 and 2^40 + 3,
    so a reduction or an accumulator narrowed to 32 bits changes the totals.
    bytes_written, unique_bytes, unique_chunks and cdc_dedup_ratio equal the
    dict's Python-int sums after every batch."""
    import chunkfs_amd as c
    ix, model = c.DedupIndex(2048), DictIndex()
    for dig, lens in totals_batches():
        insert_checked(ix, model, dig, lens)
    assert model.stats()["bytes_written"] > 2 ** 45 and model.stats()["unique_bytes"] > 2 ** 44
