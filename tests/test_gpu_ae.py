"""The AE chunker on the GPU (-m gpu): chunk lists bit-exact against
tests/ae_model.py (the rule restated on the CPU, not the kernels' bitmap form)
through every entry point -- chunk_array, device batches, async batches, the
write path (the model's StorageWriter loop), the device file layer and the
re-chunk scrubber.  Model results are computed once per (parameters, input)."""
import functools

import numpy as np
import pytest

import ae_model as ae
import oracle

pytestmark = pytest.mark.gpu

# (min, avg, max, window; None = the default)
PARAMS = [
    (64, 256, 1024, None),          # small sizes, default window
    (4096, 8192, 16384, None),      # the config-2 sizes
    (16, 64, 256, 1),               # smallest window (the direct-compare kernel)
    (100, 200, 400, 63),            # the 64-position word edge:
    (8, 128, 300, 64),              #   62 / 63 is where the kernels change,
    (8, 128, 300, 65),              #   64 / 65 where a window first spans a whole word
    (1024, 4096, 65536, 65),        # large skip, window far below min
    (16384, 65536, 524288, None),   # window wider than a 32 KiB piece
    (100, 400, 1600, 200),          # two whole words inside every window (148: one, 4767: three or more)
]
MIN_MODE_SET = 1  # this one runs in Min mode as well
CASES = [(p, ae.MAX) for p in PARAMS] + [(PARAMS[MIN_MODE_SET], ae.MIN), (PARAMS[2], ae.MIN)]
IDS = [f"{p[0]}-{p[1]}-{p[2]}-w{p[3]}-{'min' if m else 'max'}" for p, m in CASES]
_cache = {}


def chunker(p, mode):
    import chunkfs_amd as c
    key = (p, mode)
    if key not in _cache:
        _cache[key] = c.AeChunker(c.SizeParams(*p[:3]), window=p[3], mode=mode)
    return _cache[key]


@functools.lru_cache(maxsize=None)
def rand(n, seed):
    return oracle.splitmix64_bytes(n, seed)


@functools.lru_cache(maxsize=None)
def model_rand(p, mode, n, seed):
    return ae.chunk_array(rand(n, seed), *p, mode=mode)


def assert_same(gpu, ref, what=""):
    gpu = np.asarray(gpu, dtype=np.uint64).reshape(-1, 2)
    ref = np.asarray(ref, dtype=np.uint64).reshape(-1, 2)
    if gpu.shape != ref.shape or not (gpu == ref).all():
        n = min(len(gpu), len(ref))
        bad = np.nonzero((gpu[:n] != ref[:n]).any(axis=1))[0]
        i = int(bad[0]) if len(bad) else n
        pytest.fail(f"{what}: {len(gpu)} vs {len(ref)} chunks; first mismatch at #{i}: "
                    f"gpu={gpu[i].tolist() if i < len(gpu) else None} ref={ref[i].tolist() if i < len(ref) else None}")


@pytest.mark.parametrize("p,mode", CASES, ids=IDS)
def test_random_streams_bit_exact(p, mode):
    for n in [(3 << 20) + 17, 1 << 20, 100003]:
        assert_same(chunker(p, mode).chunk_array(rand(n, n + 1)), model_rand(p, mode, n, n + 1), f"{p} n={n}")


@pytest.mark.parametrize("p,mode", CASES, ids=IDS)
def test_tail_lengths(p, mode):
    mn, _, mx, _ = p
    base = rand(3 * mx + 400, 99)
    for n in list(range(0, 71)) + list(range(max(mn - 3, 0), mn + 4)) + [3 * mx + k for k in range(0, 400, 37)]:
        assert_same(chunker(p, mode).chunk_array(base[:n]), ae.chunk_array(base[:n], *p, mode=mode), f"{p} n={n}")


def _pattern(name):
    n = 600000
    i = np.arange(n)
    if name.startswith("const"):
        return np.full(n, int(name[5:], 16), dtype=np.uint8)
    if name.startswith("period"):
        k = int(name[6:])
        return np.tile(rand(k, k), n // k + 1)[:n].copy()
    if name == "3symbol":
        return (rand(n, 3) % 3).astype(np.uint8)
    return (i % 256).astype(np.uint8) if name == "ramp_up" else (255 - i % 256).astype(np.uint8)


PATTERNS = ["const00", "constAA", "constFF", "period61", "period4096", "3symbol", "ramp_up", "ramp_down"]


@pytest.mark.parametrize("name", PATTERNS)
def test_patterns_exact(name):
    """Chains that never merge (constant and periodic data) go through the
    fix-up rounds and the in-order pass; every position of constant data is an
    extremum of its window."""
    data = _pattern(name)
    for p, mode in [(PARAMS[0], ae.MAX), (PARAMS[0], ae.MIN), (PARAMS[1], ae.MAX), (PARAMS[2], ae.MAX),
                    (PARAMS[4], ae.MIN), (PARAMS[7], ae.MAX), (PARAMS[8], ae.MIN)]:
        assert_same(chunker(p, mode).chunk_array(data), ae.chunk_array(data, *p, mode=mode), f"{name} {p} mode {mode}")


def _batch(ch, bufs, lens):
    import torch
    cap = ch.batch_max_chunks(lens)
    out = torch.empty((max(cap, 1), 2), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    first = ch.chunk_batch_device([b if isinstance(b, int) else b.data_ptr() for b in bufs], lens, out.data_ptr(), cap)
    return out.cpu().numpy().astype(np.uint64), first


@pytest.mark.parametrize("pi,mode", [(0, ae.MAX), (1, ae.MIN), (2, ae.MAX), (7, ae.MAX)])
def test_ragged_device_batch(pi, mode):
    import torch
    p = PARAMS[pi]
    mn, _, mx, _ = p
    lens = [0, 5, 1 << 20, 0, 12345, 3 * mx + 1, (2 << 20) + 77, 0, mn, 700001]
    host = [rand(n, 500 + i) for i, n in enumerate(lens)]
    bufs = [torch.from_numpy(h.copy()).to("cuda:0") if len(h) else torch.empty(16, dtype=torch.uint8, device="cuda:0")
            for h in host]
    got, first = _batch(chunker(p, mode), bufs, lens)
    for i, h in enumerate(host):
        assert_same(got[first[i]:first[i + 1]], ae.chunk_array(h, *p, mode=mode), f"{p} stream {i} (len {lens[i]})")


@pytest.mark.parametrize("fill", [0xFF, 0x00])
@pytest.mark.parametrize("mode", [ae.MAX, ae.MIN])
def test_streams_end_at_their_own_length(fill, mode):
    """Three streams back to back in one allocation (16-byte starts), the bytes
    between and after them 0xFF or 0x00: a value or a window read past a
    stream's end would see them instead of the rule's zeros."""
    import torch
    lens = [70001, 65536, 4099]
    host = [rand(n, 900 + i) for i, n in enumerate(lens)]
    starts, at = [], 0
    for n in lens:
        starts.append(at)
        at = (at + n + 15) // 16 * 16 + 16
    whole = np.full(at + 4096, fill, dtype=np.uint8)
    for s, h in zip(starts, host):
        whole[s:s + len(h)] = h
    d = torch.from_numpy(whole).to("cuda:0")
    for p in (PARAMS[0], PARAMS[2], PARAMS[3], PARAMS[5], PARAMS[1]):
        got, first = _batch(chunker(p, mode), [d.data_ptr() + s for s in starts], lens)
        for i, h in enumerate(host):
            assert_same(got[first[i]:first[i + 1]], ae.chunk_array(h, *p, mode=mode),
                        f"{p} mode {mode} fill {fill:#x} stream {i}")


@pytest.mark.parametrize("pi,mode", [(0, ae.MAX), (1, ae.MAX), (1, ae.MIN), (2, ae.MAX)])
def test_write_path_is_the_storage_writer_loop(pi, mode):
    import chunkfs_amd as c
    p = PARAMS[pi]
    data = rand((3 << 20) + 999, 4242)
    ref = ae.storage_writer(data, *p, mode=mode)
    spans, _ = c.write_spans(chunker(p, mode), data)
    assert [int(x) for x in spans] == ref
    w = c.StreamWriter(chunker(p, mode))  # the same segments by hand, an empty one among them
    for off in range(0, data.size, 1 << 20):
        w.write(data[off:off + (1 << 20)])
        w.write(data[:0])
    spans2, _ = w.finish()
    assert [int(x) for x in spans2] == ref


def test_write_path_follows_each_segment_buffer_end():
    """Small segments of 3-symbol data, window 1: cuts land in the last bytes
    of a segment's buffer, where the rule reads its zero padding and values tie
    in their leading bytes -- the spans are the per-buffer loop's, not one
    chunk_data over the whole write."""
    import chunkfs_amd as c
    p = PARAMS[2]
    data = (rand(300000, 77) % 3).astype(np.uint8)
    ref = ae.storage_writer(data, *p, seg=1000)
    assert ref != [int(x) for x in ae.chunk_array(data, *p)[:, 1]]  # (the case shows the difference)
    spans, _ = c.write_spans(chunker(p, ae.MAX), data, seg_size=1000)
    assert [int(x) for x in spans] == ref


def test_async_batches_equal_the_synchronous_result():
    import torch
    p = PARAMS[1]
    ch = chunker(p, ae.MAX)
    n = (12 << 20) + 7
    data = rand(n, 31)
    buf = torch.from_numpy(data.copy()).to("cuda:0")
    cap = ch.batch_max_chunks([n])
    out = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
    sync_out = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    first = ch.chunk_batch_device([buf.data_ptr()], [n], sync_out.data_ptr(), cap)
    fs = [ch.chunk_batch_device_async([buf.data_ptr()], [n], out.data_ptr(), cap) for _ in range(7)]
    assert ch.batch_sync() == int(first[-1])
    torch.cuda.synchronize()
    for f in fs:
        assert (f == first).all()
    k = int(first[1])
    assert (out[:k] == sync_out[:k]).all()
    assert_same(sync_out[:k].cpu().numpy(), ae.chunk_array(data, *p), "12 MiB device stream")


def test_chunk_and_hash_and_store_write():
    import hashlib
    import chunkfs_amd as c
    p = PARAMS[0]
    data = rand(100003, 100004)
    chunks, dig = chunker(p, ae.MAX).chunk_and_hash(data)
    assert_same(chunks, model_rand(p, ae.MAX, 100003, 100004), "chunk_and_hash")
    for (o, ln), d in list(zip(chunks, dig))[::37]:
        assert hashlib.sha256(data[int(o):int(o + ln)].tobytes()).digest() == d.tobytes()
    store = c.ChunkStore(1 << 12, 1 << 20)
    ch2, dig2, new = store.write(chunker(p, ae.MAX), data)
    assert (ch2 == chunks).all() and (dig2 == dig).all() and new.all()
    assert (store.read(dig2) == data).all()


def test_describe_estimate_and_window():
    import chunkfs_amd as c
    ch = chunker(PARAMS[1], ae.MAX)
    assert repr(ch) == "AE, sizes: SizeParams { min: 4096, avg: 8192, max: 16384 }, window: 4767, mode: Max [MI355X gfx950]"
    assert ch.window == 4767
    assert repr(chunker(PARAMS[2], ae.MIN)).endswith("window: 1, mode: Min [MI355X gfx950]")
    assert ch.estimate_chunk_count(10 ** 7) == 10 ** 7 // 4096
    assert ch.max_chunk_count(10 ** 7) == 10 ** 7 // 4096 + 1
    dflt = c.Chunker("ae", 4096, 8192, 16384)  # cdc_create(CDC_ALGO_AE): Max mode, the default window
    assert repr(dflt) == repr(ch)
    data = rand(100003, 100004)
    assert_same(dflt.chunk_array(data), model_rand(PARAMS[1], ae.MAX, 100003, 100004), "cdc_create(CDC_ALGO_AE)")
    dflt.close()


# ---- upper layers: 4 MiB ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _four_mib():
    return rand(4 << 20, 2024)


def _file_spans(fs, h):
    import torch
    st = fs.stat(h)
    out = torch.empty(max(st["size"], 1), dtype=torch.uint8, device="cuda:0")
    spans = torch.empty((max(st["spans"], 1), 2), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert fs.read_complete_device(h, out.data_ptr(), st["size"], spans.data_ptr()) == st["size"]
    return out[:st["size"]].cpu().numpy(), spans[:st["spans"]].cpu().numpy().astype(np.uint64)


def test_file_system_with_an_ae_chunker():
    """The device file layer chunks one write_to_file as one buffer: its spans
    are the model's chunks of the call's bytes."""
    import chunkfs_amd as c
    data = _four_mib()
    p = PARAMS[1]
    fs = c.FileSystem(max_chunks=1 << 12, arena_bytes=8 << 20)
    h = fs.create_file("f", c.AeChunker(c.SizeParams(*p[:3])))
    ref = ae.chunk_array(data, *p)
    assert fs.write_to_file(h, data) == len(ref)
    back, spans = _file_spans(fs, h)
    assert (back == data).all()
    assert (fs.read_file_complete(h) == data).all()
    assert [int(x) for x in spans[:, 1]] == [int(x) for x in ref[:, 1]]


def test_rechunk_scrubber_with_an_ae_chunker():
    import chunkfs_amd as c
    data = _four_mib()
    sub = (64, 256, 1024, None)
    fs = c.FileSystem.new_with_scrubber(c.RechunkScrubber(c.AeChunker(c.SizeParams(64, 256, 1024))),
                                        max_chunks=1 << 12, arena_bytes=8 << 20, target_max_chunks=1 << 16,
                                        target_arena_bytes=8 << 20)
    h = fs.create_file("f", c.FastChunker(c.SizeParams(4096, 8192, 16384)))
    base = oracle.fastcdc(data, 4096, 8192, 16384)
    assert fs.write_to_file(h, data) == len(base)
    containers = {data[int(o):int(o + ln)].tobytes() for o, ln in base}
    keys, distinct = 0, set()
    for b in containers:
        a = np.frombuffer(b, dtype=np.uint8)
        for o, ln in ae.chunks(a, *sub):
            keys += 1
            distinct.add(b[o:o + ln])
    m = fs.scrub()
    assert m.processed_data == sum(len(b) for b in containers)
    st = fs.store.scrub_stats()
    assert st["keys"] == keys and st["target_containers"] == len(containers) and st["chunk_containers"] == 0
    assert fs.target.stats()["unique_chunks"] == len(distinct)
    assert (fs.read_file_complete(h) == data).all()


def test_cdc_fixture_measure_with_an_ae_chunker(tmp_path):
    import chunkfs_amd as c
    from chunkfs_amd import bench
    data = _four_mib()
    path = tmp_path / "data.bin"
    path.write_bytes(data.tobytes())
    fx = bench.CDCFixture(max_chunks=1 << 12, arena_bytes=8 << 20)
    r = fx.measure(bench.Dataset(str(path), "four"), c.AeChunker(c.SizeParams(4096, 8192, 16384)))
    assert r.chunker.startswith("AE, sizes: ") and r.size == data.size
    assert r.chunk_count == len(ae.chunk_array(data, *PARAMS[1]))
