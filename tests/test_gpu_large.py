"""Every layer past the 4 GiB line (-m gpu): one stream, one file and one arena
of N_BIG = 2^32 + 16 MiB + 4099 bytes, so that stream offsets, file offsets,
arena offsets, move distances and bit-mask indices all carry a non-zero high
word.  Every comparison is exact: chunk lists against the CPU oracle over the
whole list (tests/large_model.py, verify_by_pieces: restart + prefix stability
+ induction over pieces; tests/test_large_model.py holds both properties and
the verifier itself), digests against hashlib, bytes against the host copy of
the stream.  AE has no C oracle: windows of tests/ae_model.py across the line
and at 1, 2, 3 GiB, and the size-independent invariants over the whole list.

One device buffer of N_BIG splitmix64 bytes and one host copy of it serve the
whole module (fixture `big`); one N_BIG read-back buffer is shared.  Device
memory at any moment: the buffer 4.1 GiB, one arena of N_BIG + 1 GiB (the scrub
case: two of N_BIG + 64 MiB), the read-back buffer 4.1 GiB, workspaces -- under
20 GiB.  The largest segment-walk workspace at this shape (walk_sizes.
workspace_bytes, 4/8/16 KiB, one stream of N_BIG bytes): LeapCDC 3719 MiB
(16449 segments of 256 KiB); UltraCDC 1950, AE 981, Rabin 675 (32897 segments
of 128 KiB), SeqCDC 664 MiB -- test_walk_workspaces_at_this_shape pins them.

What each case reaches past 2^32:

  1 FastCDC     scan/resolve record positions, `(uint32_t)(tl - a0)` lengths and
                link[] deltas relative to a span whose base is >= 2^32; span
                counts of 32k (128 KiB spans), 65k (the 64 KiB-span variant
                512/2048/16384) and the 1 MiB-max spans; scan_exclusive /
                grid_of over them; stream ends at 2^32 - 1, 2^32, 2^32 + 1
  2 walk        Rabin / Ultra / Leap / Seq (both modes) / AE: uint32_t N[] and
                packed counts per segment with segment bases >= 2^32, the
                SeqCDC wave walk's 32-bit window offsets; fixed-size chunks
                whose offsets are i * size >= 2^32
  3 low entropy the max-cut and exact-step paths (zeros, a 61-byte period) at
                positions on both sides of the line
  4 batches     first[] and per-stream bases around a huge stream; two 4 GiB
                batches in flight
  5 SHA-256     chunk offsets >= 2^32 in sha256_kernel's block_words; the index
                counters past 2^32 bytes
  6 store       loc[], key_off[] and get_device's copy plan over an arena filled
                past 2^32; retain's move distances and `src - dst` shift > 2^32
  7 files       span offsets, pread plans (read_plan.hpp) and the verify
                kernel's first-difference offset past 2^32; containers at arena
                offsets past 2^32 (`late`)
  8 edits       splice / clone / diff (the one-bit-per-byte mask's word index
                `w * 64 + ...`) at offsets past 2^32; collect sliding `late`
                down by more than 2^32
  9 scrub       a five-group re-chunk scrub (1 GiB groups) and reads through the
                keys of containers past the line

Out of scope: host-buffer cdc_chunk_data of 4 GiB (its staging copy dominates
and it shares every kernel with case 1); chunks of 512 MiB and more (see
test_gpu_sha256_scale.py); get_to_dedup_ratio at this size; more than one GPU.

The module skips only when the device reports under 24 GiB free.

Wall times measured on an MI355X host, the oracle on 16 CPU threads.  The
fixture: device fill 0.16 s, host copy 0.41 s; the hashlib digests of the
4/8/16 KiB list (fixture `digests4`) 1.8 s.  The cases, each call alone:

  FastCDC whole list 4/8/16 0.08 s, 512/2048/16384 0.26 s, 32/128/1024 KiB 0.08 s;
  stream ends at the line 0.02 s
  walk whole list Rabin 0.29 s, Ultra 0.11 s, Leap 0.13 s, Seq 0.12 s each mode;
  fixed 0.01 s; Rabin / Seq stream ends 0.04 / 0.03 s; AE windows 0.48 s
  low entropy 0.64 s (zeros), 0.63 s (61-byte period): four whole lists each
  batches around a huge stream 0.01 s each; two batches in flight 0.02 s
  SHA-256 and index 0.09 s; store 0.14 s
  files: write 0.02 s, stat 0.01 s, range reads and the batch under 0.01 s, whole
  reads + hashes + verify 0.75 s (4.1 GiB of hashlib), snapshot / edits / collect
  0.01 s; scrub 0.19 s
  the whole module 9.5 s, 29 passed, none skipped; device memory in use peaked
  at 19.1 GiB (0.6 GiB of it before the module began)
"""
import ctypes
import gc
import time

import numpy as np
import pytest

import ae_model
import large_model as lm
import oracle
import store_model as sm
import walk_sizes as ws
from large_model import EDGE_LENS, LINE, N_BIG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 4242
MIB = 1 << 20
S4, S_SMALL_SPAN, S_BIG = (4096, 8192, 16384), (512, 2048, 16384), (32768, 131072, 1048576)
S_STORE = (16384, 65536, 262144)
PIECES = 64
SEQ_DEC = (1, 5, 50, 256)        # (mode, seq_length, jump_trigger, jump_size): SeqConfig's defaults, Decreasing
WALK = ["rabin", "ultra", "leap", "seq", "seq_dec"]
NEED_FREE = 24 << 30


# ---- plumbing ---------------------------------------------------------------------

def fill(t, n, seed):
    import torch
    from chunkfs_amd import _lib
    _lib.check(_lib.lib().cdc_fill_splitmix64_device(ctypes.c_void_p(t.data_ptr()), int(n), int(seed), None))
    torch.cuda.synchronize()


def make(algo, sizes):
    import chunkfs_amd as c
    s = c.SizeParams(*sizes)
    if algo == "fast":
        return c.FastChunker(s)
    if algo == "fixed":
        return c.FSChunker(sizes[0])
    if algo in ("seq", "seq_dec"):
        return c.SeqChunker(c.OperationMode.Decreasing if algo == "seq_dec" else c.OperationMode.Increasing, s)
    if algo == "ae":
        return c.AeChunker(s)
    return {"rabin": c.RabinChunker, "ultra": c.UltraChunker, "leap": c.LeapChunker}[algo](s)


def oracle_fn(algo, sizes):
    if algo == "fast":
        return lambda d: oracle.fastcdc(d, *sizes)
    if algo == "seq_dec":
        return lambda d: oracle.cdc("seq", d, *sizes, seqcfg=SEQ_DEC)
    if algo == "ae":
        return lambda d: ae_model.chunk_array(d, *sizes)
    return lambda d: oracle.cdc(algo, d, *sizes)


def run(ch, ptrs, lens, fn=None):
    """One device batch: (first[], the device chunk list)."""
    import torch
    cap = ch.batch_max_chunks(lens)
    out = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    first = (fn or ch.chunk_batch_device)(ptrs, lens, out.data_ptr(), cap)
    return first, out


def rows(out, a, b):
    import torch
    torch.cuda.synchronize()
    return out[int(a):int(b)].cpu().numpy().view(np.uint64)


def walk_params(ch):
    from chunkfs_amd import _lib
    v = (ctypes.c_uint64 * 9)()
    assert _lib.check(_lib.lib().cdc_debug_walk_params(ch._h, v, 9)) == 9
    return [int(x) for x in v]


def assert_walk_flags(ch, algo, sizes, lens, settled=True):
    """The debug read-outs of the walk tests: the engine's parameters and the
    batch's segment count equal the model's, the byte count is whole, and the
    fix-up rounds settled (no overflow into the in-order pass) unless the
    input is one whose chains legitimately never merge."""
    model = "seq" if algo == "seq_dec" else algo
    p = ws.params(model, *sizes, cfg=SEQ_DEC if algo == "seq_dec" else None)
    v, t = walk_params(ch), ch.last_timing()
    assert v[:7] == ws.debug_words(p) and v[7] == ws.segments(p, lens), (algo, v)
    assert t["bytes"] == sum(lens)
    assert v[8] in (0, 1, 2) and (v[8] == 2) >= (t["overflow_spans"] == 1), (algo, v, t)
    if settled:
        assert t["overflow_spans"] == 0, (algo, t)


class Big:
    def __init__(self, torch):
        t0 = time.perf_counter()
        self.torch = torch
        self.buf = torch.empty(N_BIG, dtype=torch.uint8, device=DEV)
        fill(self.buf, N_BIG, SEED)
        t1 = time.perf_counter()
        self.host = self.buf.cpu().numpy()
        self.fill_s, self.copy_s = t1 - t0, time.perf_counter() - t1
        self._lists, self._scratch = {}, None
        print(f"\n[large] fixture: fill {self.fill_s:.2f} s, host copy {self.copy_s:.2f} s")

    def fetch(self, a, b):
        return self.host[a:b]

    def scratch(self):
        """The one N_BIG read-back buffer."""
        if self._scratch is None:
            self._scratch = self.torch.empty(N_BIG, dtype=self.torch.uint8, device=DEV)
        return self._scratch

    def chunks(self, algo, sizes):
        """(device list, host rows) of the whole buffer, chunked once per rule
        and kept: the whole-list cases verify it, the others compare with it."""
        key = (algo, sizes)
        if key not in self._lists:
            ch = make(algo, sizes)
            first, out = run(ch, [self.buf.data_ptr()], [N_BIG])
            assert int(first[0]) == 0
            n = int(first[1])
            self._lists[key] = (out[:n].clone(), rows(out, 0, n))
            ch.close()
        return self._lists[key]

    def verify(self, got, algo, sizes, what):
        rep = lm.verify_by_pieces(got, N_BIG, self.fetch, oracle_fn(algo, sizes), sizes[2], pieces=PIECES, what=what)
        assert rep.compared == len(got) and rep.pieces == PIECES
        return rep


@pytest.fixture(scope="module")
def big():
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip(f"test_gpu_large needs 24 GiB of free device memory; {free >> 20} MiB are free")
    b = Big(torch)
    yield b
    b._lists.clear()
    b._scratch = b.buf = b.host = None
    del b
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _report(request):
    import torch
    t0 = time.perf_counter()
    yield
    free, total = torch.cuda.mem_get_info()
    print(f"\n[large] {request.node.name}: {time.perf_counter() - t0:.2f} s, "
          f"device memory in use {(total - free) / 2 ** 30:.1f} GiB")


class Guard:
    """A poisoned device buffer around `nbytes` at a destination misalignment."""

    def __init__(self, nbytes, shift=0):
        self.g = sm.Guarded(nbytes, 0, shift)

    @property
    def ptr(self):
        return self.g.out_ptr

    def check(self, got, want, what=""):
        a, body, z, _ = self.g.host()
        want = np.asarray(want, dtype=np.uint8)
        assert got == want.size, (what, got, want.size)
        assert (a == sm.POISON).all() and (z == sm.POISON).all() and (body[got:] == sm.POISON).all(), \
            f"{what}: wrote outside the range"
        assert np.array_equal(body[:got], want), what


def pread_checked(fs, h, offset, length, want, shift=0):
    g = Guard(length, shift)
    g.check(fs.pread_device(h, offset, length, g.ptr), want, f"pread({offset}, {length}) shift {shift}")


# ---- 0. the shape itself ----------------------------------------------------------

def test_walk_workspaces_at_this_shape():
    """The figures of the module docstring (no GPU work)."""
    mib = {}
    for algo in ws.ALGOS:
        p = ws.params(algo, *S4)
        mib[algo] = round(ws.workspace_bytes(algo, p, ws.segments(p, [N_BIG]), 1) / MIB)
    assert mib == {"rabin": 675, "ultra": 1950, "leap": 3719, "seq": 664, "ae": 981}
    assert max(mib.values()) * MIB < 4 << 30


def test_fixture_is_the_splitmix64_stream(big):
    """The device fill is the oracle's generator, and it does not repeat past 2^32."""
    assert np.array_equal(big.host[:MIB], oracle.splitmix64_bytes(MIB, SEED))
    assert not np.array_equal(big.host[LINE:LINE + MIB], big.host[:MIB])
    assert len(np.unique(big.host[N_BIG - 4099:])) > 200


# ---- 1. FastCDC, whole list ---------------------------------------------------------

@pytest.mark.parametrize("sizes", [S4, S_SMALL_SPAN, S_BIG], ids=lambda s: "-".join(map(str, s)))
def test_fastcdc_whole_list(big, sizes):
    ch = make("fast", sizes)
    first, out = run(ch, [big.buf.data_ptr()], [N_BIG])
    got = rows(out, first[0], first[1])
    if sizes == S4:
        t = ch.last_timing()
        assert t["bytes"] == N_BIG and t["overflow_spans"] == 0, t
    ch.close()
    lm.check_tiling(got, N_BIG, sizes[0], sizes[2])
    big.verify(got, "fast", sizes, f"fastcdc {sizes}")
    assert np.array_equal(got, big.chunks("fast", sizes)[1])      # a second handle gives the same list


def test_fastcdc_stream_ends_at_the_line(big):
    whole = big.chunks("fast", S4)[1]
    ch = make("fast", S4)
    for n in EDGE_LENS:
        first, out = run(ch, [big.buf.data_ptr()], [n])
        got = rows(out, first[0], first[1])
        assert ch.last_timing()["bytes"] == n
        lm.check_tiling(got, n, S4[0], S4[2])
        assert lm.verify_against_longer(got, n, whole, big.fetch, oracle_fn("fast", S4), S4[2],
                                        what=f"fastcdc n={n}") == len(got)
    ch.close()


# ---- 2. the walk chunkers, whole list --------------------------------------------

@pytest.mark.parametrize("algo", WALK)
def test_walk_whole_list(big, algo):
    ch = make(algo, S4)
    first, out = run(ch, [big.buf.data_ptr()], [N_BIG])
    assert_walk_flags(ch, algo, S4, [N_BIG])
    got = rows(out, first[0], first[1])
    ch.close()
    lm.check_tiling(got, N_BIG, S4[0], S4[2])
    big.verify(got, algo, S4, f"{algo} {S4}")
    assert np.array_equal(got, big.chunks(algo, S4)[1])


def test_fixed_whole_list(big):
    ch = make("fixed", S4)
    first, out = run(ch, [big.buf.data_ptr()], [N_BIG])
    assert ch.last_timing()["bytes"] == N_BIG
    got = rows(out, first[0], first[1])
    ch.close()
    assert np.array_equal(got, oracle.fixed(N_BIG, S4[0]))


@pytest.mark.parametrize("algo", ["rabin", "seq"])
def test_walk_stream_ends_at_the_line(big, algo):
    whole = big.chunks(algo, S4)[1]
    ch = make(algo, S4)
    for n in EDGE_LENS:
        first, out = run(ch, [big.buf.data_ptr()], [n])
        assert_walk_flags(ch, algo, S4, [n])
        got = rows(out, first[0], first[1])
        lm.check_tiling(got, n, S4[0], S4[2])
        assert lm.verify_against_longer(got, n, whole, big.fetch, oracle_fn(algo, S4), S4[2],
                                        what=f"{algo} n={n}") == len(got)
    ch.close()


def test_ae_windows_and_invariants(big):
    ch = make("ae", S4)
    first, out = run(ch, [big.buf.data_ptr()], [N_BIG])
    assert_walk_flags(ch, "ae", S4, [N_BIG])
    got = rows(out, first[0], first[1])
    ch.close()
    lm.check_tiling(got, N_BIG, S4[0], S4[2])
    fn = oracle_fn("ae", S4)
    c, k = lm.verify_window(got, N_BIG, big.fetch, fn, S4[2], LINE - 8 * MIB, 16 * MIB, what="ae across the line")
    assert LINE - 8 * MIB <= c < LINE - 8 * MIB + S4[2] and k > 1000
    for gib in (1, 2, 3):
        c, k = lm.verify_window(got, N_BIG, big.fetch, fn, S4[2], gib << 30, 4 * MIB, what=f"ae at {gib} GiB")
        assert k > 250
    # ... and the end of the list: the last 2 MiB run to N_BIG and are compared whole
    lm.verify_window(got, N_BIG, big.fetch, fn, S4[2], N_BIG - 2 * MIB, 4 * MIB, what="ae at the end")


# ---- 3. low entropy across the line ----------------------------------------------

@pytest.mark.parametrize("kind", ["zeros", "periodic61"])
def test_low_entropy_across_the_line(big, kind):
    import torch
    a, b = LINE - MIB, LINE + MIB
    patch = np.zeros(b - a, dtype=np.uint8) if kind == "zeros" else np.resize(oracle.splitmix64_bytes(61, 7), b - a)
    saved = big.host[a:b].copy()
    try:
        big.host[a:b] = patch
        big.buf[a:b].copy_(torch.from_numpy(patch).to(DEV))
        torch.cuda.synchronize()
        for algo, sizes in [("fast", S4), ("fast", S_SMALL_SPAN), ("rabin", S4), ("seq", S4)]:
            ch = make(algo, sizes)
            first, out = run(ch, [big.buf.data_ptr()], [N_BIG])
            if algo != "fast":
                assert_walk_flags(ch, algo, sizes, [N_BIG], settled=False)
            got = rows(out, first[0], first[1])
            ch.close()
            big.verify(got, algo, sizes, f"{kind} {algo} {sizes}")
            inside = got[(got[:, 0] >= np.uint64(a + sizes[2])) & (got[:, 0] + got[:, 1] <= np.uint64(b))]
            assert len(inside) > 50                                   # chunks that lie wholly in the run
    finally:
        big.host[a:b] = saved
        fill(big.buf, N_BIG, SEED)
    assert torch.equal(big.buf[a - 64:b + 64].cpu(), torch.from_numpy(big.host[a - 64:b + 64]))


# ---- 4. batch shapes around a huge stream ----------------------------------------

SMALL_LENS = (3 * MIB + 17, MIB + 13)


@pytest.fixture(scope="module")
def small():
    import torch
    o3 = 3 * MIB + 32                                  # 16-byte aligned, past the first stream
    host = oracle.splitmix64_bytes(o3 + SMALL_LENS[1] + 64, 77)
    d = torch.from_numpy(host).to(DEV)
    torch.cuda.synchronize()
    yield host, d, o3


@pytest.mark.parametrize("algo", ["fast", "rabin", "seq"])
def test_batch_around_a_huge_stream(big, small, algo):
    host, d, o3 = small
    whole = big.chunks(algo, S4)[1]
    lens = [SMALL_LENS[0], N_BIG, 0, SMALL_LENS[1]]
    ptrs = [d.data_ptr(), big.buf.data_ptr(), d.data_ptr(), d.data_ptr() + o3]
    ch = make(algo, S4)
    first, out = run(ch, ptrs, lens)
    if algo != "fast":
        assert_walk_flags(ch, algo, S4, lens)
    assert ch.last_timing()["bytes"] == sum(lens)
    ch.close()
    fn = oracle_fn(algo, S4)
    r0, r3 = fn(host[:lens[0]]), fn(host[o3:o3 + lens[3]])
    want_first = np.cumsum([0, len(r0), len(whole), 0, len(r3)]).astype(np.uint64)
    assert np.array_equal(np.asarray(first, dtype=np.uint64), want_first), (first, want_first)
    assert np.array_equal(rows(out, first[0], first[1]), r0)
    assert np.array_equal(rows(out, first[1], first[2]), whole)
    assert np.array_equal(rows(out, first[3], first[4]), r3)


def test_two_huge_batches_in_flight(big):
    whole = big.chunks("fast", S4)[1]
    ch = make("fast", S4)
    res = [run(ch, [big.buf.data_ptr()], [N_BIG], fn=ch.chunk_batch_device_async) for _ in range(2)]
    assert ch.batch_sync() == len(whole)
    for first, out in res:
        assert [int(x) for x in first] == [0, len(whole)]
        assert np.array_equal(rows(out, 0, len(whole)), whole)
    ch.close()


# ---- 5. SHA-256 and the index ----------------------------------------------------

@pytest.fixture(scope="module")
def digests4(big):
    """hashlib digests of the 4/8/16 KiB list (shared, read-only)."""
    d = lm.sha256_rows(big.host, big.chunks("fast", S4)[1])
    d.setflags(write=False)
    return d


def test_sha256_and_index_past_the_line(big, digests4):
    import torch
    import chunkfs_amd as c
    d_list, whole = big.chunks("fast", S4)
    n = len(whole)
    ch = make("fast", S4)
    dig = torch.full((n, 32), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    ch.sha256_chunks_device(big.buf.data_ptr(), d_list.data_ptr(), n, dig.data_ptr())
    torch.cuda.synchronize()
    got = dig.cpu().numpy()
    bad = np.flatnonzero((got != digests4).any(axis=1))
    assert not len(bad), f"{len(bad)} wrong digests, first at chunk {int(bad[0])} offset {int(whole[bad[0], 0])}"
    ix = c.DedupIndex(2 * n)
    assert ix.insert_device(dig.data_ptr(), d_list.data_ptr(), n) == n
    st = ix.stats()
    assert (st["unique_chunks"], st["unique_bytes"], st["chunks_written"], st["bytes_written"]) == (n, N_BIG, n, N_BIG)
    assert ix.insert_device(dig.data_ptr(), d_list.data_ptr(), n) == 0
    st = ix.stats()
    assert (st["unique_chunks"], st["unique_bytes"], st["chunks_written"], st["bytes_written"]) == \
        (n, N_BIG, 2 * n, 2 * N_BIG)
    assert st["cdc_dedup_ratio"] == 2.0
    ch.close()
    del ix


# ---- 6. the chunk store ----------------------------------------------------------

def test_store_past_the_line(big):
    import torch
    import chunkfs_amd as c
    d_list, whole = big.chunks("fast", S_STORE)
    n = len(whole)
    assert 30000 < n < 1 << 17
    ch = make("fast", S_STORE)
    dig = torch.full((n, 32), 0xA5, dtype=torch.uint8, device=DEV)
    new = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    ch.sha256_chunks_device(big.buf.data_ptr(), d_list.data_ptr(), n, dig.data_ptr())
    torch.cuda.synchronize()
    store = c.ChunkStore(1 << 18, N_BIG + (1 << 30))
    assert store.put_device(big.buf.data_ptr(), N_BIG, d_list.data_ptr(), dig.data_ptr(), n, new.data_ptr()) == n
    assert bool(new.all())
    st = store.stats()
    padded = int(((whole[:, 1] + np.uint64(15)) & ~np.uint64(15)).sum())
    assert st["arena_used"] == padded >= N_BIG and (st["unique_chunks"], st["unique_bytes"]) == (n, N_BIG)

    # the chunks from 2^32 - 1 MiB on, at two destination misalignments
    k0 = int(np.searchsorted(whole[:, 0], np.uint64(LINE - MIB)))
    a = int(whole[k0, 0])
    assert a < LINE and n - k0 > 100
    want_spans = whole[k0:] - np.array([a, 0], dtype=np.uint64)
    for shift in (1, 6):
        g = sm.Guarded(N_BIG - a, n - k0, shift)
        got = store.get_device(dig[k0:].data_ptr(), n - k0, g.out_ptr, N_BIG - a, g.spans.data_ptr())
        lo, body, hi, spans = g.host()
        assert got == N_BIG - a and (lo == sm.POISON).all() and (hi == sm.POISON).all()
        assert np.array_equal(body, big.host[a:]) and np.array_equal(spans, want_spans)

    # every chunk, compared on the device
    back = big.scratch()
    back.fill_(0xA5)
    torch.cuda.synchronize()
    assert store.get_device(dig.data_ptr(), n, back.data_ptr(), N_BIG) == N_BIG
    torch.cuda.synchronize()
    assert torch.equal(back, big.buf)

    dist = store.size_distribution(4096)
    assert sum(dist.values()) == n
    want_dist = dict(zip(*[x.tolist() for x in np.unique(whole[:, 1] // np.uint64(4096) * np.uint64(4096),
                                                         return_counts=True)]))
    assert dist == want_dist

    # keep only the chunks past the line: they slide down by more than 2^32
    k1 = int(np.searchsorted(whole[:, 0], np.uint64(LINE)))
    b = int(whole[k1, 0])
    assert store.retain_device(dig[k1:].data_ptr(), n - k1) == n - k1
    st = store.stats()
    kept = int(((whole[k1:, 1] + np.uint64(15)) & ~np.uint64(15)).sum())
    assert st["arena_used"] == kept < 17 * MIB and (st["unique_chunks"], st["unique_bytes"]) == (n - k1, N_BIG - b)
    g = sm.Guarded(N_BIG - b, n - k1, 3)
    assert store.get_device(dig[k1:].data_ptr(), n - k1, g.out_ptr, N_BIG - b, g.spans.data_ptr()) == N_BIG - b
    lo, body, hi, spans = g.host()
    assert (lo == sm.POISON).all() and (hi == sm.POISON).all() and np.array_equal(body, big.host[b:])
    assert np.array_equal(spans, whole[k1:] - np.array([b, 0], dtype=np.uint64))
    with pytest.raises(c.CdcError):                 # a dropped chunk is gone
        store.get_device(dig[:1].data_ptr(), 1, None, 0)
    ch.close()
    del store


# ---- 7, 8. the file layer --------------------------------------------------------

LATE_N = 3 * MIB + 5
EDIT_AT, EDIT_N = LINE + 12345, 4096
INS_AT, INS = LINE + 99, np.arange(7, dtype=np.uint8) + 201


def slots_of(fs, h):
    from chunkfs_amd import _lib
    n = fs.stat(h)["spans"]
    s, loc = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint64 * max(n, 1))()
    assert _lib.lib().cdc_debug_file_slots(h._fh, s, loc, n) == n
    return list(s)[:n], list(loc)[:n]


class TestFiles:
    @pytest.fixture(scope="class")
    def fsys(self, big):
        import chunkfs_amd as c
        ch = make("fast", S_STORE)
        fs = c.FileSystem(max_chunks=1 << 20, arena_bytes=N_BIG + (1 << 30))
        filler = fs.create_file("filler", ch)
        t0 = time.perf_counter()
        spans = fs.write_to_file(filler, big.buf)
        print(f"\n[large] write of filler: {time.perf_counter() - t0:.2f} s")
        late_data = oracle.splitmix64_bytes(LATE_N, SEED + 1)
        late = fs.create_file("late", ch)
        fs.write_to_file(late, late_data)
        state = {"fs": fs, "ch": ch, "filler": filler, "late": late, "late_data": late_data, "spans": spans}
        yield state
        state.clear()
        del fs, filler, late
        ch.close()
        gc.collect()

    def test_write_and_stat(self, big, fsys):
        fs = fsys["fs"]
        whole = big.chunks("fast", S_STORE)[1]
        st = fs.stat(fsys["filler"])
        assert (st["size"], st["spans"]) == (N_BIG, len(whole)) and fsys["spans"] == len(whole)
        st = fs.stat(fsys["late"])
        assert st["size"] == LATE_N
        _, locs = slots_of(fs, fsys["late"])
        assert len(locs) == st["spans"] and min(locs) >= N_BIG          # containers past 2^32 in the arena
        _, locs = slots_of(fs, fsys["filler"])
        assert max(locs) >= LINE

    def test_range_reads(self, big, fsys):
        fs, h, host = fsys["fs"], fsys["filler"], big.host
        pread_checked(fs, h, LINE - 5000, 10000, host[LINE - 5000:LINE + 5000])
        pread_checked(fs, h, LINE, 1, host[LINE:LINE + 1])
        pread_checked(fs, h, N_BIG - 100, 150, host[N_BIG - 100:])               # clipped
        pread_checked(fs, h, N_BIG, 10, host[:0])
        whole = big.chunks("fast", S_STORE)[1]
        k = int(np.searchsorted(whole[:, 0], np.uint64(LINE + 3 * MIB)))
        at = int(whole[k, 0]) + int(whole[k, 1]) // 2 + 1                          # mid-chunk past the line
        for shift in (0, 1, 7, 13):
            pread_checked(fs, h, at, MIB, host[at:at + MIB], shift)
        pread_checked(fs, fsys["late"], 0, LATE_N, fsys["late_data"], 5)

    def test_batched_range_reads(self, big, fsys):
        fs, h, late, host = fsys["fs"], fsys["filler"], fsys["late"], big.host
        reqs = [(h, 12345, 70000), (h, LINE - 70001, 140002), (late, 17, 2 * MIB), (h, LINE + 5 * MIB + 3, 300001),
                (h, (2 << 30) - 9, 65536), (h, N_BIG - 4099, 8192), (late, LATE_N - 5, 5), (h, LINE - 1, 2)]
        guards = [Guard(ln, i % 4) for i, (_, _, ln) in enumerate(reqs)]
        got = fs.pread_batch_device([(f, off, ln, g.ptr) for (f, off, ln), g in zip(reqs, guards)])
        for (f, off, ln), g, k in zip(reqs, guards, got):
            src = fsys["late_data"] if f is late else host
            g.check(k, src[off:off + ln], f"batched pread({off}, {ln})")

    def test_whole_reads_hashes_and_verify(self, big, fsys):
        import torch
        fs, h = fsys["fs"], fsys["filler"]
        whole = big.chunks("fast", S_STORE)[1]
        n = fs.stat(h)["spans"]
        assert n == len(whole)
        back = big.scratch()
        back.fill_(0xA5)
        d_spans = torch.full((n, 2), -1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        assert fs.read_complete_device(h, back.data_ptr(), N_BIG, d_spans.data_ptr()) == N_BIG
        torch.cuda.synchronize()
        assert torch.equal(back, big.buf)
        assert np.array_equal(d_spans.cpu().numpy().view(np.uint64), whole)
        g = Guard(LATE_N, 3)
        g.check(fs.read_complete_device(fsys["late"], g.ptr, LATE_N), fsys["late_data"], "late, whole")

        # read_from_file's loop: whole spans, at most one segment each, to the end
        r = fs.open_file_readonly("filler")
        seg = torch.empty(fs.seg_size, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        cur = calls = 0
        while True:
            k = fs.read_device(r, seg.data_ptr(), fs.seg_size)
            if k == 0:
                break
            assert fs.seg_size - S_STORE[2] < k <= fs.seg_size or cur + k == N_BIG
            torch.cuda.synchronize()
            assert torch.equal(seg[:k], big.buf[cur:cur + k]), f"segment at {cur}"
            cur += k
            calls += 1
        assert cur == N_BIG and fs.stat(r)["cursor"] == N_BIG and calls >= N_BIG // fs.seg_size

        assert np.array_equal(fs.hashes(h), lm.sha256_rows(big.host, whole))

        assert fs.verify_device(h, big.buf.data_ptr(), N_BIG) == (True, None)
        assert fs.verify_device(h, back.data_ptr(), N_BIG) == (True, None)
        back[LINE + 7] ^= 0x40
        torch.cuda.synchronize()
        assert fs.verify_device(h, back.data_ptr(), N_BIG) == (False, LINE + 7)
        assert fs.verify_device(h, big.buf.data_ptr(), LINE + 1) == (False, LINE + 1)   # only the sizes differ

    def test_snapshot_edit_diff_and_collect(self, big, fsys):
        fs, h, late, host = fsys["fs"], fsys["filler"], fsys["late"], big.host
        n_spans = fs.stat(h)["spans"]
        assert fs.clone_file("filler", "snap") == n_spans
        snap = fs.open_file_readonly("snap")
        new = host[EDIT_AT:EDIT_AT + EDIT_N] ^ np.uint8(0xFF)

        def edited(a, b):
            """[a, b) of the file after the pwrite."""
            w = host[a:b].copy()
            lo, hi = max(a, EDIT_AT), min(b, EDIT_AT + EDIT_N)
            if lo < hi:
                w[lo - a:hi - a] = new[lo - EDIT_AT:hi - EDIT_AT]
            return w

        s = fs.pwrite(h, EDIT_AT, new)
        assert (s.size_before, s.size_after) == (N_BIG, N_BIG) and s.resync_offset >= EDIT_AT + EDIT_N
        assert fs.stat(h)["size"] == N_BIG
        d = fs.diff(snap, h)
        assert d.ranges.tolist() == [[EDIT_AT, EDIT_N]] and d.bytes_differing == EDIT_N
        assert (d.size_a, d.size_b) == (N_BIG, N_BIG)
        # Only the pieces the two tables do not share are read.  The splice re-chunks from the span that holds
        # EDIT_AT - 8 until a new cut falls on an old one; content-defined cuts realign within a few chunks, and
        # 16 max-size chunks (4 MiB, a thousandth of the file) is far more than that yet far from "everything".
        assert EDIT_N <= d.bytes_compared <= 16 * S_STORE[2] and d.bytes_shared >= N_BIG - 16 * S_STORE[2]
        t = fs.diff(snap, h, tables_only=True)
        assert t.bytes_compared == 0 and len(t.ranges) >= 1
        lo, hi = int(t.ranges[0, 0]), int(t.ranges[-1, 0] + t.ranges[-1, 1])
        assert lo <= EDIT_AT and EDIT_AT + EDIT_N <= hi and hi - lo <= 16 * S_STORE[2]
        assert int(t.ranges[:, 1].sum()) == t.bytes_differing == N_BIG - t.bytes_shared
        a = EDIT_AT - 70000
        pread_checked(fs, h, a, 150000, edited(a, a + 150000), 3)
        pread_checked(fs, snap, a, 150000, host[a:a + 150000], 1)          # the snapshot keeps the old bytes

        # insert, delete, truncate: stat and the last 64 KiB (and the edit's surroundings) against the model
        K = 65536
        s = fs.insert(h, INS_AT, INS)
        assert (s.size_before, s.size_after) == (N_BIG, N_BIG + 7) and fs.stat(h)["size"] == N_BIG + 7
        pread_checked(fs, h, N_BIG + 7 - K, K, edited(N_BIG - K, N_BIG), 2)
        w = np.concatenate([edited(INS_AT - 5000, INS_AT), INS, edited(INS_AT, INS_AT + 20000)])
        pread_checked(fs, h, INS_AT - 5000, w.size, w, 1)
        s = fs.delete_range(h, INS_AT, 7)
        assert (s.size_before, s.size_after) == (N_BIG + 7, N_BIG) and fs.stat(h)["size"] == N_BIG
        pread_checked(fs, h, N_BIG - K, K, edited(N_BIG - K, N_BIG), 5)
        pread_checked(fs, h, INS_AT - 5000, 25007, edited(INS_AT - 5000, INS_AT + 20007), 0)
        assert fs.diff(snap, h).ranges.tolist() == [[EDIT_AT, EDIT_N]]     # back to the one edit
        s = fs.truncate(h, LINE + 1)
        assert (s.size_before, s.size_after) == (N_BIG, LINE + 1) and fs.stat(h)["size"] == LINE + 1
        pread_checked(fs, h, LINE + 1 - K, K + 10, host[LINE + 1 - K:LINE + 1], 7)
        assert fs.diff(snap, h).ranges.tolist() == [[LINE + 1, N_BIG - LINE - 1]]

        # remove both big files and collect: `late` slides down by more than 2^32
        _, before = slots_of(fs, late)
        used = fs.store.stats()["arena_used"]
        fs.remove_file("filler")
        fs.remove_file("snap")
        r = fs.collect()
        st = fs.store.stats()
        _, after = slots_of(fs, late)
        assert r["arena_used_before"] == used > N_BIG and r["arena_used_after"] == st["arena_used"] < 16 * MIB
        assert r["containers_before"] > r["containers_after"] == len(set(after))
        assert r["bytes_moved"] >= LATE_N and r["groups_direct"] + r["groups_bounced"] >= 1
        assert min(before) >= N_BIG and max(after) < 16 * MIB
        assert min(b - a for a, b in zip(after, before)) > LINE
        g = Guard(LATE_N, 9)
        g.check(fs.read_complete_device(late, g.ptr, LATE_N), fsys["late_data"], "late after the collect")
        pread_checked(fs, fs.open_file_readonly("late"), 12345, MIB, fsys["late_data"][12345:12345 + MIB], 1)
        assert fs.list_files() == ["late"]


# ---- 9. scrub past the line ------------------------------------------------------

def test_scrub_past_the_line(big):
    import torch
    import chunkfs_amd as c
    sub = make("fast", S4)
    base = make("fast", S_STORE)
    fs = c.FileSystem.new_with_scrubber(c.RechunkScrubber(sub), max_chunks=1 << 18, arena_bytes=N_BIG + (64 << 20),
                                        target_max_chunks=1 << 21, target_arena_bytes=N_BIG + (64 << 20))
    h = fs.create_file("filler", base)
    fs.write_to_file(h, big.buf)
    m = fs.scrub()
    assert (m.processed_data, m.data_left) == (N_BIG, 0) and m.running_time > 0
    x = fs.store.scrub_stats()
    assert x["chunk_containers"] == 0 and x["target_bytes"] == N_BIG, x
    host = big.host
    pread_checked(fs, h, LINE - 5000, 10000, host[LINE - 5000:LINE + 5000], 1)
    pread_checked(fs, h, LINE, 1, host[LINE:LINE + 1])
    pread_checked(fs, h, N_BIG - 100, 150, host[N_BIG - 100:], 3)
    pread_checked(fs, h, LINE + 3 * MIB + 77, MIB, host[LINE + 3 * MIB + 77:LINE + 4 * MIB + 77], 7)
    back = big.scratch()
    back.fill_(0xA5)
    torch.cuda.synchronize()
    assert fs.read_complete_device(h, back.data_ptr(), N_BIG) == N_BIG
    torch.cuda.synchronize()
    assert torch.equal(back, big.buf)
    del fs, h
    sub.close()
    base.close()
    gc.collect()
