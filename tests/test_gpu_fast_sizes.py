"""FastCDC over its whole size range on the GPU (-m gpu): the size table of
tests/fast_sizes.py (every round(log2 avg) from 8 to 22, spans of 2^16 to 2^24
bytes, odd sizes, avg on either side of a rounding point) through the host
path with the one-launch kernel on and off, ragged device batches, the forced
resolve paths, the write path, async bursts and chunk_and_hash.

Every comparison is bit-exact against the oracle (oracle.fastcdc /
oracle.fs_write; parity vs the fastcdc crate is unpinned: GEAR placeholder).
The engine's record cap and span count must equal the plain-Python model's
(fast_sizes.params), and which calls the one-launch kernel takes is asserted
from cdc_debug_host_stats.  tests/test_fast_sizes_model.py (no GPU) guards the
table and the references used here.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import fast_sizes as fs
import oracle

pytestmark = pytest.mark.gpu

_cache = {}
_ENV = {"small": {}, "pipeline": {"CHUNKFS_AMD_SMALL": "0"}}


def _create(sizes, env):
    """A handle created with `env` set (read once at cdc_create)."""
    import chunkfs_amd as c
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return c.FastChunker(c.SizeParams(*sizes))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def chunker(sizes, path="small"):
    """path "small": the default handle; "pipeline": CHUNKFS_AMD_SMALL=0, every
    call takes the scan + resolve pipeline (fastcdc.hip)."""
    key = (tuple(sizes), path)
    if key not in _cache:
        _cache[key] = _create(sizes, _ENV[path])
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_cached_handles():
    yield
    for ch in _cache.values():
        ch.close()
    _cache.clear()


def assert_same(got, ref, what):
    got = np.asarray(got, dtype=np.uint64).reshape(-1, 2)
    ref = np.asarray(ref, dtype=np.uint64).reshape(-1, 2)
    if got.shape != ref.shape or not (got == ref).all():
        n = min(len(got), len(ref))
        bad = np.nonzero((got[:n] != ref[:n]).any(axis=1))[0]
        i = int(bad[0]) if len(bad) else n
        pytest.fail(f"{what}: {len(got)} vs {len(ref)} chunks; first mismatch at #{i}: "
                    f"gpu={got[i].tolist() if i < len(got) else None} ref={ref[i].tolist() if i < len(ref) else None}")


def _streams(case):
    """(what, data, reference) of every single stream of a case: the three
    inputs, the threshold lengths on random and on zero bytes, the further
    lengths for the one-launch kernel, the rounding probes."""
    out = [(name, fs.data_of(case, name), fs.ref(case, name)) for name in ("random", "zeros", "zero_region")]
    for name in ("random", "zeros"):
        for n in fs.edge_lengths(case):
            out.append((f"{name}[:{n}]", fs.data_of(case, name, n), fs.ref(case, name, n)))
    for n in fs.SMALL_EXTRA.get(fs.sizes_of(case), []):
        d, r = fs.extra(case, n)
        out.append((f"extra {n}", d, r))
    for kind, (d, _) in fs.rounding_probes(case).items():  # a hit at exactly the odd position
        out.append((f"rounding probe {kind}", d, oracle.fastcdc(d, *fs.sizes_of(case))))
    return out


def _device(torch, a):
    if len(a) == 0:
        return torch.empty(16, dtype=torch.uint8, device="cuda:0")
    return torch.from_numpy(np.array(a)).to("cuda:0")  # (a copy: the shared inputs are read-only)


def _batch(torch, ch, bufs, lens, fn=None):
    cap = ch.batch_max_chunks(lens)
    out = torch.empty((max(cap, 1), 2), dtype=torch.int64, device="cuda:0")
    first = (fn or ch.chunk_batch_device)([b.data_ptr() for b in bufs], lens, out.data_ptr(), cap)
    return out, first


def _rows(torch, out, first, i):
    torch.cuda.synchronize()
    return out[int(first[i]):int(first[i + 1])].cpu().numpy().view(np.uint64)


# ---- 1. chunk_array on host buffers -------------------------------------------

@pytest.mark.parametrize("path", ["small", "pipeline"])
@pytest.mark.parametrize("case", fs.CASES, ids=fs.case_id)
def test_host_buffers_bit_exact_and_small_kernel_use(case, path):
    """Every single stream of the case through cdc_chunk_data."""
    import chunkfs_amd as c
    sizes, p = fs.sizes_of(case), fs.params(*fs.sizes_of(case))
    ch = chunker(sizes, path)
    assert "FastCDC (2020), sizes: SizeParams { min: %d, avg: %d, max: %d }" % sizes in repr(ch)
    for what, data, ref in _streams(case):
        before = c.host_stats(ch)
        got = ch.chunk_array(data)
        after = c.host_stats(ch)
        assert_same(got, ref, f"{sizes} {path} {what}")
        took = after["small_calls"] - before["small_calls"]
        want = 1 if path == "small" and fs.small_eligible(p, len(data)) else 0
        assert took == want, (sizes, path, what, len(data), "small kernel calls", took, "model", want)
        assert after["guard_trips"] == 0


# ---- 2. device batches; the engine's parameters against the model -------------

@pytest.mark.parametrize("case", fs.CASES, ids=fs.case_id)
def test_device_batch_and_engine_parameters(case):
    import torch
    from chunkfs_amd import _lib
    sizes, p = fs.sizes_of(case), fs.params(*fs.sizes_of(case))
    ch = chunker(sizes, "pipeline")
    L = _lib.lib()
    assert L.cdc_debug_record_cap(ch._h) == p.cap
    names = ["random", "zeros", "zero_region"]
    arrays = [fs.data_of(case, n) for n in names] + [np.empty(0, dtype=np.uint8)]
    bufs = [_device(torch, a) for a in arrays]
    lens = [len(a) for a in arrays]
    out, first = _batch(torch, ch, bufs, lens)
    assert int(first[0]) == 0 and int(first[4]) == int(first[3])
    for i, n in enumerate(names):
        assert_same(_rows(torch, out, first, i), fs.ref(case, n), f"{sizes} batch stream {n}")
    # one random stream: spans and record density as the model says
    out, first = _batch(torch, ch, bufs[:1], lens[:1])
    assert_same(_rows(torch, out, first, 0), fs.ref(case, "random"), f"{sizes} single random stream")
    counts = np.empty(fs.span_count(p, lens[:1]) + 8, dtype=np.uint32)
    got = _lib.check(L.cdc_debug_copy(ch._h, 0, ctypes.c_void_p(counts.ctypes.data), counts.nbytes))
    assert got % 4 == 0 and got // 4 == fs.span_count(p, lens[:1]), (sizes, got // 4, "spans; model",
                                                                    fs.span_count(p, lens[:1]))
    counts = counts[:got // 4]
    t = ch.last_timing()
    assert t["path"] == 0 and t["bytes"] == case.n
    assert t["overflow_spans"] == int((counts > p.cap).sum())
    if case.avg <= 1024:
        assert t["overflow_spans"] > 0, sizes
    else:
        assert t["overflow_spans"] == 0, sizes
        assert t["candidates"] == int(counts.sum())


def test_wide_max_over_avg_crosses_overflowed_spans():
    """fs.WIDE_CASE: about every second span of random bytes overflows the
    scan's list, so chains keep crossing between record lists and the exact
    walk from the bytes.  With 24 spans, none overflowing is a 2^-22 event and
    all of them a 2^-21 one."""
    import torch
    from chunkfs_amd import _lib
    case = fs.WIDE_CASE
    sizes, p = fs.sizes_of(case), fs.params(*fs.sizes_of(case))
    ch = chunker(sizes, "pipeline")
    assert _lib.lib().cdc_debug_record_cap(ch._h) == p.cap
    data = fs.data_of(case, "random")
    buf = _device(torch, data)
    out, first = _batch(torch, ch, [buf], [case.n])
    assert_same(_rows(torch, out, first, 0), fs.ref(case, "random"), f"{sizes} device")
    t = ch.last_timing()
    assert 0 < t["overflow_spans"] < fs.span_count(p, [case.n])
    assert_same(ch.chunk_array(fs.data_of(case, "zero_region")), fs.ref(case, "zero_region"), f"{sizes} host")


# ---- 3. forced resolve paths ---------------------------------------------------

@pytest.mark.parametrize("diag", [1, 2])
@pytest.mark.parametrize("sizes", fs.RESOLVE_CASES, ids=lambda s: "-".join(map(str, s)))
def test_forced_resolve_paths(sizes, diag):
    """CHUNKFS_AMD_DIAG 1 (walks start at the span start: stale entries, the
    settle and the look-back's re-walk) and 2 (every wave takes the dense
    path), the one-launch kernel off, at spans of 2^19, 2^22 and 2^24 bytes and
    at the odd triple."""
    import torch
    case = fs.case_of(sizes)
    ch = _create(sizes, {"CHUNKFS_AMD_DIAG": str(diag), "CHUNKFS_AMD_SMALL": "0"})
    try:
        for name in ("random", "zeros", "zero_region"):
            assert_same(ch.chunk_array(fs.data_of(case, name)), fs.ref(case, name), f"diag={diag} {sizes} {name}")
            if diag == 1 and name == "zeros" and case.max & 1:
                # cuts at k * max, max odd: no span but the first starts at a
                # chunk start, so every later span's guessed walk is re-walked
                assert ch.last_timing()["fixup_iterations"] > 0
        names = ["zero_region", "random", "zeros"]
        arrays = [fs.data_of(case, n) for n in names]
        bufs = [_device(torch, a) for a in arrays]
        out, first = _batch(torch, ch, bufs, [len(a) for a in arrays])
        for i, n in enumerate(names):
            assert_same(_rows(torch, out, first, i), fs.ref(case, n), f"diag={diag} {sizes} batch stream {n}")
    finally:
        ch.close()


# ---- 4. write path -------------------------------------------------------------

def _write_inputs(case):
    rnd = fs.data_of(case, "random")
    half = (case.n // 2) | 1
    tail = np.concatenate([rnd[:half], np.zeros(case.n - half, dtype=np.uint8)])
    return {"random": rnd, "random_then_zeros": tail}


@pytest.mark.parametrize("sizes", fs.WRITE_CASES, ids=lambda s: "-".join(map(str, s)))
def test_write_path_1mib_segments(sizes):
    """cdc_fs_write in 1 MiB segments == the oracle's StorageWriter loop == the
    chunks of the whole write.  random_then_zeros ends in max cuts: at max =
    16 MiB the reference's carried chunk spans 16 segments."""
    import chunkfs_amd as c
    case = fs.case_of(sizes)
    ch = chunker(sizes)
    for name, data in _write_inputs(case).items():
        spans, secs = c.write_spans(ch, data)
        ref_spans, _ = oracle.fs_write("fast", data, *sizes)
        whole = fs.ref(case, "random")[:, 1] if name == "random" else oracle.fastcdc(data, *sizes)[:, 1]
        assert spans.tolist() == ref_spans.tolist() == whole.tolist(), (sizes, name)
        assert int(spans.sum()) == case.n and secs > 0
        if name == "random_then_zeros" and case.n - ((case.n // 2) | 1) > case.max + 64:
            # (the chunk that runs into the zeros, or the one after a cut in
            # their first 63 bytes, finds no hit and has more than max left)
            assert case.max in spans[:-1].tolist()


def test_write_path_streaming_odd_segments():
    """cdc_write_begin / _segment / _finish in 300001-byte segments at
    (1 MiB, 4 MiB, 16 MiB)."""
    import chunkfs_amd as c
    sizes = fs.WRITE_CASES[0]
    case = fs.case_of(sizes)
    ch = chunker(sizes)
    for name, data in _write_inputs(case).items():
        w = c.StreamWriter(ch)
        for off in range(0, case.n, 300001):
            w.write(data[off:off + 300001])
        spans, _ = w.finish()
        ref_spans, _ = oracle.fs_write("fast", data, *sizes, seg_size=300001)
        assert spans.tolist() == ref_spans.tolist(), (sizes, name)
        assert int(spans.sum()) == case.n


def test_write_path_carries_a_max_chunk_across_device_windows():
    """The write path chunks one device window (fs.write_window_bytes(), read
    from host_path.hpp: 256 MiB) at a time and carries the window's last chunk to
    the front of the next one (room: max + 16 bytes); segments inside a window
    carry nothing.  So only a write longer than a window reaches the carry, and
    no setting makes the window smaller: this input is window + 20 MiB.  A zero
    run across the window boundary makes the carried chunk a full 16 MiB max
    cut; the spans must be the chunks of the whole write."""
    import chunkfs_amd as c
    sizes = fs.WRITE_CASES[0]
    case = fs.case_of(sizes)
    window = fs.write_window_bytes()
    n = window + (20 << 20) + 4321
    data = oracle.splitmix64_bytes(n, fs.SEED + 2)
    data[window - (30 << 20) + 77:window + (3 << 20) + 5] = 0
    ch = chunker(sizes)
    w = c.StreamWriter(ch)
    drained = []
    for off in range(0, n, 1 << 20):
        w.write(data[off:off + (1 << 20)])
        drained.append(w.drain())
    spans, _ = w.finish()
    assert any(d.size for d in drained)  # the first window was chunked before the end of the write
    spans = np.concatenate(drained + [spans])
    whole = oracle.fastcdc(data, *sizes)
    assert spans.tolist() == whole[:, 1].tolist()
    # the carried chunk: the one that holds the window's last byte is a max cut
    k = int(np.searchsorted(whole[:, 0], window, side="right")) - 1
    assert int(whole[k, 1]) == case.max and int(whole[k, 0]) < window < int(whole[k, 0]) + case.max


# ---- 5. async bursts ------------------------------------------------------------

@pytest.mark.parametrize("sizes", fs.ASYNC_CASES, ids=lambda s: "-".join(map(str, s)))
def test_async_burst_of_four(sizes):
    """Four cdc_chunk_batch_device_async batches of more than 8 MiB each (so
    they are in flight together), ended by cdc_batch_sync."""
    import torch
    case = fs.case_of(sizes)
    ch = chunker(sizes, "pipeline")
    big_n = max(case.n, (9 << 20) + 12345)
    big, big_ref = (fs.data_of(case, "random"), fs.ref(case, "random")) if big_n == case.n else fs.extra(case, big_n)
    streams = {"big": (big, big_ref), "empty": (np.empty(0, dtype=np.uint8), np.zeros((0, 2), np.uint64))}
    for name in ("random", "zeros", "zero_region"):
        streams[name] = (fs.data_of(case, name), fs.ref(case, name))
    bufs = {k: _device(torch, d) for k, (d, _) in streams.items()}
    shapes = [["big"], ["zeros", "big", "empty"], ["zero_region", "empty", "big", "random"], ["big", "zero_region"]]
    res = []
    for names in shapes:
        lens = [len(streams[k][0]) for k in names]
        assert sum(lens) > 8 << 20
        out, first = _batch(torch, ch, [bufs[k] for k in names], lens, ch.chunk_batch_device_async)
        res.append((names, out, first))
    assert ch.batch_sync() == int(res[-1][2][-1])
    for names, out, first in res:
        assert int(first[0]) == 0
        for i, k in enumerate(names):
            assert_same(_rows(torch, out, first, i), streams[k][1], f"{sizes} async {names} stream {k}")
    assert ch.batch_sync() == 0


# ---- 6. chunk_and_hash ------------------------------------------------------------

def test_chunk_and_hash_multi_mib_chunks():
    """(1 MiB, 4 MiB, 16 MiB): ten chunks of several MiB each, so the SHA-256
    kernel's longest-first claim order has few, huge entries."""
    sizes = (1048576, 4194304, 16777216)
    case = fs.case_of(sizes)
    ch = chunker(sizes)
    for name in ("random", "zero_region"):
        data = fs.data_of(case, name)
        chunks, digests = ch.chunk_and_hash(data)
        assert_same(chunks, fs.ref(case, name), f"{sizes} chunk_and_hash {name}")
        for (o, ln), dg in zip(chunks.tolist(), digests):
            assert dg.tobytes() == hashlib.sha256(data[o:o + ln].tobytes()).digest(), (name, o, ln)
