"""The one-launch FastCDC kernel (chunkfs_amd/csrc/small.hip) stage by stage
and on device input (-m gpu).

Every chunk list is compared bit-exactly with oracle.fastcdc, and every call is
asserted to have been taken by the one-launch kernel (cdc_debug_host_stats:
one more small call, and as many fallbacks as the model predicts).  The scan
stage -- per-block record counts, records, precomputed truncated results, the
device copy of a host input -- is read back through cdc_debug_copy (what 2..7,
include/chunkfs_amd_debug.h) and compared with the numpy model of
tests/small_model.py.  On a chunk-list mismatch the failure message names the
first block whose count or records differ from the model, or says that the scan
stage was right, so a red run names the stage.

tests/test_small_model.py (no GPU) proves that the model's chain equals the
oracle on every input used here and that each input reaches the path it was
chosen for.  By the model's counts, the inputs reach:

  a  truncated results known in the record's own block / the next block /
     only the last one: 288 / 146 / 0 (4096 set), 1638 / 263 / 0 (1024),
     759 / 167 / 0 (1000), 0 / 130 / 67 (32768); 30, 47, 54 and 3 heads; max-cut
     runs of 19, 34, 36 and 2;
  b  per set, 3 streams whose last start is the tail chunk and 130 with a live
     chunk in the end regime; 141 lengths across a block and a piece edge;
  c  trunc_load's guarded branch in 62 of 133 calls of either zero stream and
     in 56 of 133 calls of the record two blocks before its region;
  e  4 / 5 records in a lane, 256 / 257 in a block, 2048 / 2049 in a call;
  f  100, 150 and 639 heads in 3, 4 and 11 link rounds; 3093 entries wanted
     where 3072 fit.
"""
import ctypes

import numpy as np
import pytest

import fast_sizes as fs
import oracle
import small_model as sm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_handles = {}
_dev = {}


def chunker(sizes, gear=None):
    """The default handle of a size set (one per GEAR table)."""
    import chunkfs_amd as c
    key = (tuple(sizes), gear is not None)
    if key not in _handles:
        ch = c.FastChunker(c.SizeParams(*sizes))
        if gear is not None:
            ch.set_gear(gear)
        _handles[key] = ch
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for ch in _handles.values():
        ch.close()
    _handles.clear()
    _dev.clear()


def device_buffer(key, data):
    """`data` in device memory (kept for the module: the sweeps share it)."""
    import torch
    if key not in _dev:
        _dev[key] = torch.from_numpy(np.array(data)).to(DEV)
    return _dev[key]


def _stats(ch):
    import chunkfs_amd as c
    st = c.host_stats(ch)
    return st["small_calls"], st["small_fallbacks"], st["guard_trips"]


def readout(ch, what, dtype, count):
    """cdc_debug_copy of the last one-launch call; None when the library says
    the last call was not one (a fallback, a device-input call for the copy)."""
    from chunkfs_amd import _lib
    arr = np.empty(max(count, 1), dtype=dtype)
    got = _lib.lib().cdc_debug_copy(ch._h, what, ctypes.c_void_p(arr.ctypes.data), count * arr.itemsize)
    if got < 0:
        return None
    assert got == count * arr.itemsize, (what, got, count)
    return arr[:count]


def stage_report(ch, model):
    counts = readout(ch, 2, np.uint32, model.blocks)
    regions = readout(ch, 3, np.uint64, model.blocks * sm.BLOCK_REC_CAP)
    if counts is None or regions is None:
        return "no read-out: the call fell back to the pipeline"
    return sm.first_difference(model, counts, regions)


def check_chunks(ch, got, ref, model, what):
    got = np.asarray(got, dtype=np.uint64).reshape(-1, 2)
    if got.shape != ref.shape or not (got == ref).all():
        k = min(len(got), len(ref))
        bad = np.nonzero((got[:k] != ref[:k]).any(axis=1))[0]
        i = int(bad[0]) if bad.size else k
        pytest.fail(f"{what}: {len(got)} chunks for {len(ref)}; first mismatch at #{i}: "
                    f"gpu={got[i].tolist() if i < len(got) else None} ref={ref[i].tolist() if i < len(ref) else None}; "
                    + stage_report(ch, model()))


class Out:
    """One device chunk list for a whole test."""

    def __init__(self, ch, nmax):
        import torch
        self.cap = ch.batch_max_chunks([nmax])
        self.t = torch.empty((max(self.cap, 1), 2), dtype=torch.int64, device=DEV)


def device_call(ch, out, ptr, n, fallbacks=0):
    """One single-stream cdc_chunk_batch_device call on device memory at ptr;
    the kernel took it (and fell back as often as expected)."""
    s0 = _stats(ch)
    first = ch.chunk_batch_device([ptr], [n], out.t.data_ptr(), out.cap)
    s1 = _stats(ch)
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (1, fallbacks), ("small calls / fallbacks", n, s0, s1)
    if not fallbacks:
        assert ch.last_timing()["path"] == 1, n
    return out.t[:int(first[1])].cpu().numpy().view(np.uint64)


def host_call(ch, data, fallbacks=0):
    s0 = _stats(ch)
    got = ch.chunk_array(data)
    s1 = _stats(ch)
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (1, fallbacks, 0), ("small calls / fallbacks", s0, s1)
    return got


def check_scan_stage(ch, model, what, host_data=None):
    """Counts, records and truncated results of the last call against the model."""
    counts = readout(ch, 2, np.uint32, model.blocks)
    regions = readout(ch, 3, np.uint64, model.blocks * sm.BLOCK_REC_CAP)
    assert counts is not None and regions is not None, (what, "no read-out after a one-launch call")
    want = model.block_counts()
    assert counts.tolist() == want.tolist(), (what, sm.first_difference(model, counts, regions))
    for b in range(model.blocks):
        got = regions[b * sm.BLOCK_REC_CAP:b * sm.BLOCK_REC_CAP + int(want[b])]
        exp = model.block_regions(b)
        # position and flags; then each truncated byte: the model's value, or
        # "unknown" only where the model says the last block alone can know it
        assert (got == exp).all(), (what, sm.first_difference(model, counts, regions))
    copy = readout(ch, 4, np.uint8, model.n)
    if host_data is None:
        assert copy is None, (what, "a device-input call leaves no device copy to read")
    else:
        assert copy is not None and (copy == host_data[:model.n]).all(), (what, "device copy of the host input")


# ---- a. the scan stage against the model ----------------------------------------

@pytest.mark.parametrize("name", sm.SCAN_DATA)
@pytest.mark.parametrize("sizes", sm.SCAN_SETS, ids=sm.set_id)
def test_scan_stage_matches_model(sizes, name):
    scan = sm.scan_of(sizes, name)
    data, n = scan.buf, scan.buf.size
    assert fs.small_eligible(scan.p, n)
    model = scan.model()
    assert not model.fallback()
    ref = sm.ref_of(scan, n, (sizes, name))
    ch = chunker(sizes)
    out = Out(ch, n)
    buf = device_buffer((sizes, name), data)
    got = device_call(ch, out, buf.data_ptr(), n)
    check_chunks(ch, got, ref, lambda: model, (sizes, name, "device input"))
    check_scan_stage(ch, model, (sizes, name, "device input"))
    got = host_call(ch, data)
    check_chunks(ch, got, ref, lambda: model, (sizes, name, "host input"))
    check_scan_stage(ch, model, (sizes, name, "host input"), host_data=data)


@pytest.mark.parametrize("sizes", sm.SCAN_SETS, ids=sm.set_id)
def test_host_copy_follows_alternating_buffers(sizes):
    """Two different buffers of one length alternated on one handle, the order
    swapped at every lap of the pinned ring: every ring slot is used again with
    the other bytes, and the device copy is the call's."""
    ch = chunker(sizes)
    pairs = [(name, sm.scan_of(sizes, name)) for name in ("random", "random2")]
    models = {name: scan.model() for name, scan in pairs}
    slots = sm.ring_slots()
    for turn in range(2 * slots + 1):
        name, scan = pairs[(turn + turn // slots) & 1]
        got = host_call(ch, scan.buf)
        check_chunks(ch, got, sm.ref_of(scan, scan.buf.size, (sizes, name)), lambda: models[name],
                     (sizes, name, "turn", turn))
        check_scan_stage(ch, models[name], (sizes, name, "turn", turn), host_data=scan.buf)


# ---- b. stream-end sweeps on device input ---------------------------------------

@pytest.mark.parametrize("kind", ["end", "block_edge", "piece_edge"])
@pytest.mark.parametrize("sizes", sm.SCAN_SETS, ids=sm.set_id)
def test_stream_end_sweep_device_input(sizes, kind):
    scan = sm.scan_of(sizes, "random")
    ch = chunker(sizes)
    out = Out(ch, scan.buf.size)
    buf = device_buffer((sizes, "random"), scan.buf)
    for n in sm.sweep_lengths(sizes)[kind]:
        got = device_call(ch, out, buf.data_ptr(), n)
        check_chunks(ch, got, sm.ref_of(scan, n, (sizes, "random")), lambda: scan.model(n), (sizes, kind, n))


# ---- c. trunc_load's guarded branch ---------------------------------------------

@pytest.mark.parametrize("sizes,k", sm.GUARD_ZERO, ids=lambda v: sm.set_id(v) if isinstance(v, tuple) else str(v))
def test_guarded_load_zero_streams(sizes, k):
    lens = sm.guard_zero_lengths(sizes, k)
    scan = sm.zeros_scan(sizes, max(lens))
    ch = chunker(sizes)
    out = Out(ch, max(lens))
    buf = device_buffer(("zeros", max(lens)), scan.buf)
    for n in lens:
        got = device_call(ch, out, buf.data_ptr(), n)
        check_chunks(ch, got, sm.ref_of(scan, n, (sizes, "zeros")), lambda: scan.model(n), (sizes, "zeros", n))


def test_guarded_load_record_two_blocks_before_its_region():
    scan, s, lens = sm.guard_random()
    sizes = scan.sizes
    ch = chunker(sizes)
    out = Out(ch, max(lens))
    buf = device_buffer(("guard_random",), scan.buf)
    for n in lens:
        got = device_call(ch, out, buf.data_ptr(), n)
        check_chunks(ch, got, sm.ref_of(scan, n, (sizes, "guard_random")), lambda: scan.model(n), (sizes, s, n))
    n = lens[len(lens) // 2]
    device_call(ch, out, buf.data_ptr(), n)
    check_scan_stage(ch, scan.model(n), (sizes, "guard_random", n))   # s: left to the last block


# ---- d. alignment and surroundings ----------------------------------------------

@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("sizes", sm.SCAN_SETS, ids=sm.set_id)
def test_alignment_and_surroundings(sizes, fill):
    """The stream inside a larger tensor whose other bytes (64 before, at least
    256 after, the same allocation) are all `fill`.  cdc_chunk_batch_device
    takes 16-byte aligned streams only (include/chunkfs_amd.h), so of the
    offsets 0..15 the offsets 1..15 must be refused before any launch; the
    stream is moved through every 16-byte position of a 256-byte line
    instead (offsets 0, 16, .. 240)."""
    import torch
    from chunkfs_amd import _lib
    scan = sm.scan_of(sizes, "random")
    src = device_buffer((sizes, "random"), scan.buf)
    ch = chunker(sizes)
    lens = sm.align_lengths(sizes)
    out = Out(ch, max(lens))
    big = torch.empty(64 + 256 + max(lens) + 256, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 256 == 0
    for off in range(1, 16):
        s0 = _stats(ch)
        with pytest.raises(_lib.CdcError, match="16-byte aligned"):
            ch.chunk_batch_device([big.data_ptr() + 64 + off], [lens[0]], out.t.data_ptr(), out.cap)
        assert _stats(ch) == s0
    for off in range(0, 256, 16):
        for n in lens:
            big.fill_(fill)
            big[64 + off:64 + off + n] = src[:n]
            got = device_call(ch, out, big.data_ptr() + 64 + off, n)
            check_chunks(ch, got, sm.ref_of(scan, n, (sizes, "random")), lambda: scan.model(n),
                         (sizes, "offset", off, "fill", fill, n))


# ---- e. record budgets at their edges -------------------------------------------

@pytest.mark.parametrize("budget,at", [("lane", sm.LANE_HITS), ("block", sm.BLOCK_REC_CAP), ("call", sm.REC_CAP)])
def test_record_budget_edges(budget, at):
    """GEAR[0] = 0 and zero runs placed by the model: exactly the budget (no
    fallback, the stage read-out equal to the model) and one record more
    (exactly one fallback); exact chunk lists either way, on both inputs."""
    cases = sm.budget_cases()
    for t in (at, at + 1):
        name = f"{budget}_{t}"
        scan = cases[name]
        model = scan.model()
        fb = 1 if model.fallback() else 0
        assert fb == (t > at) and model.record_fallback() == (budget if fb else None)
        ch = chunker(scan.sizes, scan.gear)
        n = scan.buf.size
        ref = sm.ref_of(scan, n, (name, "gear0"))
        out = Out(ch, n)
        buf = device_buffer((name,), scan.buf)
        got = device_call(ch, out, buf.data_ptr(), n, fallbacks=fb)
        check_chunks(ch, got, ref, lambda: model, (name, "device input"))
        if not fb:
            check_scan_stage(ch, model, (name, "device input"))
        else:
            assert readout(ch, 2, np.uint32, model.blocks) is None   # the pipeline answered: nothing to read
        got = host_call(ch, scan.buf, fallbacks=fb)
        check_chunks(ch, got, ref, lambda: model, (name, "host input"))
        if not fb:
            check_scan_stage(ch, model, (name, "host input"), host_data=scan.buf)


# ---- f. entry budget and link rounds --------------------------------------------

def test_entry_budget_exceeded_by_truncated_hits():
    """Dense records whose links are truncated hits: every record budget holds,
    the entries run out, exactly one fallback per call, exact chunks."""
    scan = sm.budget_cases()["entries_over"]
    model = scan.model()
    assert model.record_fallback() is None and model.chain_fallback()
    ch = chunker(scan.sizes, scan.gear)
    n = scan.buf.size
    ref = sm.ref_of(scan, n, ("entries_over", "gear0"))
    out = Out(ch, n)
    got = device_call(ch, out, device_buffer(("entries_over",), scan.buf).data_ptr(), n, fallbacks=1)
    check_chunks(ch, got, ref, lambda: model, "entries_over, device input")
    got = host_call(ch, scan.buf, fallbacks=1)
    check_chunks(ch, got, ref, lambda: model, "entries_over, host input")


@pytest.mark.parametrize("sizes,n", sm.ENTRY_CASES, ids=lambda v: sm.set_id(v) if isinstance(v, tuple) else str(v))
def test_entry_budget_and_link_rounds(sizes, n):
    """Zero streams (default GEAR): every start but offset 0 is a head, added
    in runs of at most 64 per round.  (Heads of double the entry budget are out
    of an eligible stream's reach: test_small_model.py.)"""
    scan = sm.zeros_scan(sizes, n)
    model = scan.model()
    assert not model.fallback() and model.chain().max_run > sm.RUN_LEN and model.link_stage()[1] > 1
    ch = chunker(sizes)
    out = Out(ch, n)
    buf = device_buffer(("zeros", n), scan.buf)
    got = device_call(ch, out, buf.data_ptr(), n)
    check_chunks(ch, got, sm.ref_of(scan, n, (sizes, "zeros")), lambda: model, (sizes, "zeros", n, "device"))
    check_scan_stage(ch, model, (sizes, "zeros", n))
    got = host_call(ch, scan.buf)
    check_chunks(ch, got, sm.ref_of(scan, n, (sizes, "zeros")), lambda: model, (sizes, "zeros", n, "host"))


# ---- g. scratch history ---------------------------------------------------------

@pytest.mark.parametrize("order", ["host-host", "device-host", "host-device"])
def test_short_call_after_long_call(order):
    """A 3 MiB call, then a 40 KiB call on the same handle: the short call's
    stages and chunks are its own, and the long call's records and copy bytes
    still lie in the scratch beyond it."""
    sizes = sm.SCAN_SETS[3]
    long_scan, short_scan = sm.scan_of(sizes, "random"), sm.scan_of(sizes, "random2")
    n_long, n_short = long_scan.buf.size, 40 * sm.KIB
    long_model, short_model = long_scan.model(), short_scan.model(n_short)
    ch = chunker(sizes)
    out = Out(ch, n_long)
    first, second = order.split("-")

    def call(kind, scan, n, model, tag):
        if kind == "host":
            got = host_call(ch, scan.buf[:n])
        else:
            got = device_call(ch, out, device_buffer((sizes, tag), scan.buf).data_ptr(), n)
        check_chunks(ch, got, sm.ref_of(scan, n, (sizes, tag)), lambda: model, (order, tag, n))
        check_scan_stage(ch, model, (order, tag, n), host_data=scan.buf if kind == "host" else None)

    call(first, long_scan, n_long, long_model, "random")
    call(second, short_scan, n_short, short_model, "random2")
    # the whole scratch: the short call's blocks first, the long call's beyond
    counts = readout(ch, 5, np.uint32, sm.MAX_BLOCKS)
    regions = readout(ch, 6, np.uint64, sm.MAX_BLOCKS * sm.BLOCK_REC_CAP)
    want = long_model.block_counts()
    assert counts[:short_model.blocks].tolist() == short_model.block_counts().tolist()
    assert counts[short_model.blocks:long_model.blocks].tolist() == want[short_model.blocks:].tolist()
    for b in range(short_model.blocks, long_model.blocks):
        got = regions[b * sm.BLOCK_REC_CAP:b * sm.BLOCK_REC_CAP + int(want[b])]
        assert (got == long_model.block_regions(b)).all(), (order, "block", b)
    if first == "host" and second == "host":
        copy = readout(ch, 7, np.uint8, n_long)
        assert (copy[:n_short] == short_scan.buf[:n_short]).all()
        edge = -(-n_short // sm.PIECE) * sm.PIECE        # (a wave copies its whole 4 KiB piece)
        assert (copy[edge:] == long_scan.buf[edge:]).all()


# ---- the end regime in front of a piece the stream never reaches ----------------

def test_end_region_in_front_of_an_unloaded_piece():
    """GEAR[0] = 0: a record whose region of zero bytes (a hit at its first
    position) ends with the stream just below a 4 KiB piece edge, so that the
    block evaluates it from the 64 bytes in front of a piece that holds no
    byte of the stream.  Each call follows a 4 MiB call of bytes that are
    never zero: 128 blocks leave such bytes in the LDS of the CUs they ran on,
    and a block that did not load those 64 bytes reads a result other than 0
    (the scan-stage comparison was red with 63 before the fix in small.hip)."""
    cases = sm.piece_end_cases()
    scan0 = cases[0][1]
    ch = chunker(scan0.sizes, scan0.gear)
    noise = oracle.splitmix64_bytes(fs.SMALL_MAX_BYTES, 77)
    noise[noise == 0] = 1
    nbuf = device_buffer(("noise",), noise)
    out = Out(ch, fs.SMALL_MAX_BYTES)
    for name, scan, n, c in cases:
        device_call(ch, out, nbuf.data_ptr(), fs.SMALL_MAX_BYTES)
        model = scan.model(n)
        ref = sm.ref_of(scan, n, (name, "gear0"))
        buf = device_buffer((name,), scan.buf)
        got = device_call(ch, out, buf.data_ptr(), n)
        check_chunks(ch, got, ref, lambda: model, (name, "device input"))
        check_scan_stage(ch, model, (name, "device input"))
        got = host_call(ch, scan.buf[:n])
        check_chunks(ch, got, ref, lambda: model, (name, "host input"))
        check_scan_stage(ch, model, (name, "host input"), host_data=scan.buf)
