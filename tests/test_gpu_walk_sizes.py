"""The segment-walk chunkers over their whole size range and batch shapes on
the GPU (-m gpu): the table of tests/walk_sizes.py (segments of 4 KiB to 4 MiB,
chunks that run over hundreds of segments, sizes at the top of uint32_t,
rounding points, degenerate and odd triples) through device batches, the host
path, forced fix-up schedules and the write path; batches of more than 2^16
segments (the gated output without the fused end kernel); the unfused end
(CHUNKFS_AMD_WALK_FUSED=0) at the block edges of its kernels; the quiet-run
summary off (CHUNKFS_AMD_QUIET=0).

Every comparison is bit-exact against the oracle (oracle.cdc / oracle.fs_write)
or, for AE, tests/ae_model.py.  What the engine derived from the sizes, the
segment count of each batch and how the batch ended (cdc_debug_walk_params)
must equal the plain-Python model's (walk_sizes.params), so each test also
asserts that it is in the regime it names.  tests/test_walk_sizes_model.py (no
GPU) guards the table.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle
import walk_sizes as ws
from gen_golden import make_input
from test_gpu_walk import BYTE_PERIOD, BYTE_SIZES, repeat_run_stream

pytestmark = pytest.mark.gpu

END_FUSED, END_GATED, END_UNGATED = 0, 1, 2   # cdc_debug_walk_params, value 8
_cache = {}


def make(case, env=None):
    """A handle of the case's rule and sizes, created with `env` set (the
    engine reads its variables once, at creation)."""
    import chunkfs_amd as c
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = c.SizeParams(*ws.sizes_of(case))
        if case.algo == "seq":
            cfg = case.cfg or (0,)
            return c.SeqChunker(cfg[0], s, c.SeqConfig(*cfg[1:])) if len(cfg) > 1 else c.SeqChunker(cfg[0], s)
        if case.algo == "ae":
            return c.AeChunker(s, window=case.cfg)
        return {"rabin": c.RabinChunker, "ultra": c.UltraChunker, "leap": c.LeapChunker}[case.algo](s)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def chunker(case, env=None):
    key = (case, tuple(sorted((env or {}).items())))
    if key not in _cache:
        _cache[key] = make(case, env)
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_cached_handles():
    yield
    for ch in _cache.values():
        ch.close()
    _cache.clear()
    _big.clear()


def walk_params(ch):
    from chunkfs_amd import _lib
    v = (ctypes.c_uint64 * 9)()
    assert _lib.check(_lib.lib().cdc_debug_walk_params(ch._h, v, 9)) == 9
    return [int(x) for x in v]


def assert_same(got, ref, what):
    got = np.asarray(got, dtype=np.uint64).reshape(-1, 2)
    ref = np.asarray(ref, dtype=np.uint64).reshape(-1, 2)
    if got.shape != ref.shape or not (got == ref).all():
        n = min(len(got), len(ref))
        bad = np.nonzero((got[:n] != ref[:n]).any(axis=1))[0]
        i = int(bad[0]) if len(bad) else n
        pytest.fail(f"{what}: {len(got)} vs {len(ref)} chunks; first mismatch at #{i}: "
                    f"gpu={got[i].tolist() if i < len(got) else None} ref={ref[i].tolist() if i < len(ref) else None}")


def _device(torch, a):
    if len(a) == 0:
        return torch.empty(16, dtype=torch.uint8, device="cuda:0")
    return torch.from_numpy(np.array(a)).to("cuda:0")  # (a copy: the shared inputs are read-only)


def _batch(torch, ch, ptrs, lens, fn=None):
    cap = ch.batch_max_chunks(lens)
    out = torch.empty((max(cap, 1), 2), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    first = (fn or ch.chunk_batch_device)(ptrs, lens, out.data_ptr(), cap)
    return out, first


def _rows(torch, out, first, i):
    torch.cuda.synchronize()
    return out[int(first[i]):int(first[i + 1])].cpu().numpy().view(np.uint64)


def _check_first(first, n):
    f = np.asarray(first, dtype=np.uint64)
    assert len(f) == n + 1 and int(f[0]) == 0 and (f[1:] >= f[:-1]).all()


# ---- 1. the engine's parameters and device batches ------------------------------

def test_debug_export_refuses_other_handles():
    import chunkfs_amd as c
    from chunkfs_amd import _lib
    ch = c.FastChunker(c.SizeParams(4096, 8192, 16384))
    v = (ctypes.c_uint64 * 9)()
    assert _lib.lib().cdc_debug_walk_params(ch._h, v, 9) == _lib.CDC_EINVAL
    assert b"not a segment-walk handle" in _lib.lib().cdc_last_error()
    ch.close()


@pytest.mark.parametrize("case", ws.CASES, ids=ws.case_id)
def test_engine_parameters_and_device_batches(case):
    """cdc_debug_walk_params equals the model field by field; one ragged batch
    of the case's inputs and an empty stream, then the random input alone."""
    import torch
    p = ws.params(case.algo, *ws.sizes_of(case), cfg=case.cfg)
    ch = chunker(case)
    what = ws.case_id(case)
    assert walk_params(ch)[:7] == ws.debug_words(p), what
    names = ws.input_names(case)
    arrays = [ws.inputs(case)[n] for n in names] + [np.empty(0, dtype=np.uint8)]
    bufs = [_device(torch, a) for a in arrays]
    lens = [len(a) for a in arrays]
    out, first = _batch(torch, ch, [b.data_ptr() for b in bufs], lens)
    _check_first(first, len(lens))
    assert int(first[-1]) == int(first[-2])
    assert walk_params(ch)[7] == ws.segments(p, lens), what
    for i, n in enumerate(names):
        assert_same(_rows(torch, out, first, i), ws.ref(case, n), f"{what} batch stream {n}")
    out, first = _batch(torch, ch, [bufs[0].data_ptr()], lens[:1])
    v = walk_params(ch)
    assert v[:7] == ws.debug_words(p) and v[7] == ws.segments(p, lens[:1]), what
    assert v[8] in (END_FUSED, END_UNGATED)       # (a batch of at most 2^16 segments, the fused end on)
    assert_same(_rows(torch, out, first, 0), ws.ref(case, "random"), f"{what} single random stream")
    t = ch.last_timing()
    assert t["bytes"] == case.n and (v[8] == END_UNGATED) >= (t["overflow_spans"] == 1)


# ---- 2. the host path -----------------------------------------------------------

@pytest.mark.parametrize("case", ws.CASES, ids=ws.case_id)
def test_host_buffers_bit_exact(case):
    ch = chunker(case)
    for name in ws.input_names(case):
        assert_same(ch.chunk_array(ws.inputs(case)[name]), ws.ref(case, name), f"{ws.case_id(case)} host {name}")


# ---- 3. forced fix-up schedules on the new regimes ------------------------------

@pytest.mark.parametrize("ahead", ["0,64", "16,1"])
@pytest.mark.parametrize("case", ws.SCHEDULE_CASES, ids=ws.case_id)
def test_forced_schedules(case, ahead):
    """Run-ahead re-walks from round 0 (64 segments) and plain Jacobi that may
    run out of rounds into the in-order pass, at the default segment sizes of
    a small-segment and a 4 MiB-segment case per rule.  The zero-region input
    makes both cross chunks that span many segments."""
    import torch
    ch = chunker(case, {"CHUNKFS_AMD_AHEAD": ahead})
    p = ws.params(case.algo, *ws.sizes_of(case), cfg=case.cfg)
    what = f"{ws.case_id(case)} ahead={ahead}"
    assert walk_params(ch)[:7] == ws.debug_words(p), what
    for name in ["zero_region", "random"] + (["pattern"] if case.pattern else []):
        data = ws.inputs(case)[name]
        buf = _device(torch, data)
        out, first = _batch(torch, ch, [buf.data_ptr()], [case.n])
        assert_same(_rows(torch, out, first, 0), ws.ref(case, name), f"{what} {name}")
        t, v = ch.last_timing(), walk_params(ch)
        print(f"{what} {name}: fixup_iterations {t['fixup_iterations']} overflow_spans {t['overflow_spans']} end {v[8]}")
        assert (v[8] == END_UNGATED) >= (t["overflow_spans"] == 1)
        # The rounds must run where a walk's guessed start cannot be a true
        # chunk start: SeqCDC cuts a zero run only at max, counted from where
        # the run's first chunk began (a content-defined cut in the random
        # bytes before it), while a segment deep in the run is walked from a
        # multiple of max, the warm-up or more before it -- in the
        # small-segment case, where the run (1.5 max) holds such a multiple
        # and the segments after it.  Elsewhere
        # (runs that cut at min or after 64 equal blocks, whatever the phase;
        # 4 MiB segments, whose warm-up reaches back past the run's start)
        # the guessed chains can be right at once: no assertion.
        if case.algo == "seq" and case.group == "small" and name == "zero_region":
            assert t["fixup_iterations"] > 0, what


# ---- 4. the write path ----------------------------------------------------------

@pytest.mark.parametrize("case", ws.WRITE_CASES, ids=ws.case_id)
def test_write_path_1mib_segments(case):
    """cdc_fs_write in 1 MiB segments == the oracle's StorageWriter loop == the
    chunks of the whole write.  random_then_run ends in max cuts: the carried
    chunk spans 16 segments."""
    import chunkfs_amd as c
    ch = chunker(case)
    sizes = ws.sizes_of(case)
    for name, (data, whole) in ws.write_inputs(case).items():
        spans, secs = c.write_spans(ch, data)
        ref_spans, _ = oracle.fs_write(case.algo, data, *sizes)
        assert spans.tolist() == ref_spans.tolist() == whole[:, 1].tolist(), (ws.case_id(case), name)
        assert int(spans.sum()) == case.n and secs > 0
        if name == "random_then_run":
            assert case.max == 16 << 20 and case.max in spans[:-1].tolist()


def test_write_path_streaming_odd_segments():
    """cdc_write_begin / _segment / _finish in 300001-byte segments at SeqCDC
    (64 KiB, 1 MiB, 16 MiB)."""
    import chunkfs_amd as c
    case = ws.WRITE_CASES[0]
    ch = chunker(case)
    for name, (data, _) in ws.write_inputs(case).items():
        w = c.StreamWriter(ch)
        for off in range(0, case.n, 300001):
            w.write(data[off:off + 300001])
        spans, _ = w.finish()
        ref_spans, _ = oracle.fs_write(case.algo, data, *ws.sizes_of(case), seg_size=300001)
        assert spans.tolist() == ref_spans.tolist(), (ws.case_id(case), name)
        assert int(spans.sum()) == case.n


# ---- 5. more than 2^16 segments in a batch --------------------------------------
# Handles are created with CHUNKFS_AMD_WALK="12,2" (4 KiB segments, a 2-avg
# warm-up): at the default segment sizes (128 / 256 KiB) the per-segment bitmaps
# and LeapCDC tables of a batch of 66000 streams would take several GiB
# (test_walk_sizes_model.py::test_workspace_stays_under_a_gib).

BIG_ENV = {"CHUNKFS_AMD_WALK": "%d,%d" % ws.BIG_WALK}
_big = {}


def _big_device(torch, key, lens, pieces):
    """One device buffer with every stream 16-byte aligned in it; pieces[i] =
    the host bytes of stream i.  Returns (buffer, device address per stream).
    One buffer is kept at a time."""
    if _big.get("device key") != key:
        _big.pop("device", None)
        starts, pos = [], 0
        for n in lens:
            starts.append(pos)
            pos += (n + 15) // 16 * 16
        img = np.zeros(pos + 16, dtype=np.uint8)
        for i, n in enumerate(lens):
            if n:
                img[starts[i]:starts[i] + n] = pieces[i]
        dev = torch.from_numpy(img).to("cuda:0")
        _big["device key"], _big["device"] = key, (dev, np.array(starts, dtype=np.uint64) + np.uint64(dev.data_ptr()))
    return _big["device"]


def _big_refs(case, key, lens, pieces):
    """Per stream, the reference chunks (every stream, none sampled), as one
    array in batch order and first[]."""
    k = (case, key)
    if k not in _big:
        refs = [ws.reference(case, pieces[i]) if n else np.zeros((0, 2), np.uint64) for i, n in enumerate(lens)]
        first = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.uint64)
        _big[k] = (np.concatenate(refs), first)
    return _big[k]


def _assert_batch(torch, out, first, ref_rows, ref_first, lens, what):
    _check_first(first, len(lens))
    if not (np.asarray(first, dtype=np.uint64) == ref_first).all():
        i = int(np.nonzero(np.asarray(first, dtype=np.uint64) != ref_first)[0][0])
        pytest.fail(f"{what}: first[{i}] = {int(first[i])}, reference {int(ref_first[i])} (stream {i - 1}, "
                    f"{lens[i - 1]} bytes)")
    torch.cuda.synchronize()
    assert_same(out[:int(first[-1])].cpu().numpy().view(np.uint64), ref_rows, what)


@pytest.mark.parametrize("algo", ws.ALGOS)
def test_more_than_65536_segments(algo):
    """About 66000 streams, more than 2^16 segments: finish_kernel does not
    take the batch, so the output is the gated launch_emit behind the first
    fix-up round, and prefix_kernel's carry loop runs over more than 256 block
    sums.  Then the same batch trimmed to exactly 2^16 segments (the fused end)
    and to 2^16 + 1.  The rule's sizes and the long streams' bytes (ws.BIG) are
    those under which the first round changes no exit
    (test_walk_sizes_model.py::test_big_batch_settles_in_the_first_round)."""
    import torch
    sizes, kind = ws.BIG[algo]
    lens, pieces = ws.big_batch(kind)
    case = ws.big_case(algo)
    p = ws.params(algo, *sizes, walk=ws.BIG_WALK)
    ch = chunker(case, BIG_ENV)
    assert walk_params(ch)[:7] == ws.debug_words(p)
    dev, ptrs = _big_device(torch, kind, lens, pieces)
    ref_rows, ref_first = _big_refs(case, kind, lens, pieces)
    out, first = _batch(torch, ch, ptrs, lens)
    total = int(first[len(lens)])
    _assert_batch(torch, out, first, ref_rows, ref_first, lens, f"{algo} {len(lens)} streams")
    v, t = walk_params(ch), ch.last_timing()
    assert v[7] == ws.segments(p, lens) > ws.FINISH_MAX
    assert v[8] == END_GATED, (algo, v, t)
    assert t["fixup_iterations"] > 0                      # the 2-avg warm-up leaves entries to fix
    assert total == len(ref_rows) and (np.asarray(first[-5:]) == total).all()
    for want, end in ((ws.FINISH_MAX, END_FUSED), (ws.FINISH_MAX + 1, END_GATED)):
        tl = ws.trim_to_segments(lens, p.seg_log2, want)
        k = len(tl)
        last = ws.reference(case, pieces[k - 1][:tl[-1]])
        rows = np.concatenate([ref_rows[:int(ref_first[k - 1])], last])
        rf = np.concatenate([ref_first[:k], [ref_first[k - 1] + np.uint64(len(last))]]).astype(np.uint64)
        out, first = _batch(torch, ch, ptrs[:k], tl)
        _assert_batch(torch, out, first, rows, rf, tl, f"{algo} trimmed to {want} segments")
        v = walk_params(ch)
        assert v[7] == want and v[8] == end, (algo, want, v)


@pytest.mark.parametrize("algo", ws.ALGOS)
def test_more_than_65536_segments_async(algo):
    """The same batch twice through cdc_chunk_batch_device_async on a handle
    with three contexts (CHUNKFS_AMD_WALK_CTX=3), ended by cdc_batch_sync."""
    import torch
    kind = ws.BIG[algo][1]
    lens, pieces = ws.big_batch(kind)
    case = ws.big_case(algo)
    ch = chunker(case, dict(BIG_ENV, CHUNKFS_AMD_WALK_CTX="3"))
    assert sum(lens) > 8 << 20                            # (smaller batches complete in their call)
    dev, ptrs = _big_device(torch, kind, lens, pieces)
    ref_rows, ref_first = _big_refs(case, kind, lens, pieces)
    res = [_batch(torch, ch, ptrs, lens, ch.chunk_batch_device_async) for _ in range(2)]
    assert ch.batch_sync() == len(ref_rows)
    for out, first in res:
        _assert_batch(torch, out, first, ref_rows, ref_first, lens, f"{algo} async")
    assert ch.batch_sync() == 0


def _periodic_pieces(algo):
    lens, pieces = ws.big_batch("random")
    pieces = list(pieces)
    for i in [i for i, n in enumerate(lens) if n >= 20000][::3]:
        pieces[i] = make_input("periodic", lens[i], BYTE_PERIOD[algo])
    return lens, pieces


@pytest.mark.parametrize("algo", sorted(BYTE_PERIOD))
def test_more_than_65536_segments_non_settling_chains(algo):
    """Every third long stream replaced by the periodic input whose chains
    never merge under the rule (test_gpu_walk.BYTE_PERIOD, at its sizes 256 /
    1024 / 4096), plain Jacobi only (CHUNKFS_AMD_AHEAD="16,1"): the rounds run
    out, the in-order pass finishes the call and the output is the ungated
    launch_emit.  (No such period is known for AE: not in this test.)"""
    import torch
    case = ws.big_case(algo, BYTE_SIZES)
    p = ws.params(algo, *BYTE_SIZES, walk=ws.BIG_WALK)
    ch = chunker(case, dict(BIG_ENV, CHUNKFS_AMD_AHEAD="16,1"))
    lens, pieces = _periodic_pieces(algo)
    dev, ptrs = _big_device(torch, ("periodic", algo), lens, pieces)
    ref_rows, ref_first = _big_refs(case, "periodic", lens, pieces)
    out, first = _batch(torch, ch, ptrs, lens)
    _assert_batch(torch, out, first, ref_rows, ref_first, lens, f"{algo} periodic long streams")
    v, t = walk_params(ch), ch.last_timing()
    assert v[7] == ws.segments(p, lens) > ws.FINISH_MAX
    assert v[8] == END_UNGATED and t["overflow_spans"] == 1, (algo, v, t)
    _big.pop((case, "periodic"))                          # (one rule's only)


# ---- 6. the unfused end; the quiet-run summary off ------------------------------

FUSED_CASES = [ws.Case("rabin", 4096, 8192, 16384, 0, None, "fused", None),     # bitmap mode
               ws.Case("rabin", 16, 64, 256, 0, None, "fused", None)]           # byte mode


def _edge_lengths(p, segs, rng):
    """Stream lengths with exactly `segs` segments: a three-segment stream,
    an empty one and one-segment streams of 1 to 2^seg_log2 bytes."""
    seg = 1 << p.seg_log2
    lens = [int(x) for x in rng.integers(1, seg + 1, segs - 3)]
    lens.insert(len(lens) // 2, 2 * seg + 5)
    lens.insert(1, 0)
    assert ws.segments(p, lens) == segs
    return lens


@pytest.mark.parametrize("case", FUSED_CASES, ids=ws.case_id)
def test_unfused_end_at_block_edges(case):
    """CHUNKFS_AMD_WALK_FUSED=0 (sum_kernel / prefix_kernel / emit_kernel and
    D2H copies instead of finish_kernel) at 255, 256, 257 and 513 segments:
    chunks and first[] identical to the default handle's and to the oracle.
    4 KiB segments (CHUNKFS_AMD_WALK="12,8") keep the batches small."""
    import torch
    env = {"CHUNKFS_AMD_WALK": "12,8"}
    p = ws.params(case.algo, *ws.sizes_of(case), walk=(12, 8))
    default, unfused = chunker(case, env), chunker(case, dict(env, CHUNKFS_AMD_WALK_FUSED="0"))
    rng = np.random.default_rng(513)
    ends = set()
    for segs in (255, 256, 257, 513):
        lens = _edge_lengths(p, segs, rng)
        offs = np.concatenate([[0], np.cumsum(lens)])
        host = oracle.splitmix64_bytes(int(offs[-1]) + 16, segs)
        pieces = [host[offs[i]:offs[i] + n] for i, n in enumerate(lens)]
        bufs = [_device(torch, a) for a in pieces]
        ptrs = [b.data_ptr() for b in bufs]
        refs = [ws.reference(case, a) for a in pieces]
        res = []
        for ch, name in ((default, "default"), (unfused, "unfused")):
            out, first = _batch(torch, ch, ptrs, lens)
            _check_first(first, len(lens))
            v = walk_params(ch)
            assert v[:7] == ws.debug_words(p) and v[7] == segs
            assert (v[8] == END_FUSED) == (name == "default") or v[8] == END_UNGATED, (name, segs, v)
            ends.add((name, v[8]))
            for i in range(len(lens)):
                assert_same(_rows(torch, out, first, i), refs[i], f"{ws.case_id(case)} {name} {segs} segments stream {i}")
            res.append((np.asarray(first).copy(), out[:int(first[-1])].cpu().numpy()))
        assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
    assert ("unfused", END_FUSED) not in ends and ("default", END_GATED) not in ends


@pytest.mark.parametrize("algo", ["rabin", "ultra"])
def test_quiet_summary_off_equals_default(algo):
    """CHUNKFS_AMD_QUIET=0 (no quiet-run summary in the workspace) over long
    zero / constant / 8-byte-periodic runs: the default handle's chunks."""
    case = ws.Case(algo, 4096, 8192, 16384, 0, None, "quiet", None)
    data = repeat_run_stream(12 << 20, 35)
    got_default = chunker(case).chunk_array(data)
    got_off = chunker(case, {"CHUNKFS_AMD_QUIET": "0"}).chunk_array(data)
    assert_same(got_off, got_default, f"{algo} quiet=0 vs default")
    assert_same(got_off, ws.reference(case, data), f"{algo} quiet=0 vs oracle")
