"""Call-sequence parity on the GPU (-m gpu): a handle's results must not depend
on what it ran before.

Each test runs one scripted sequence of tests/history_harness.py -- different
entry points, shapes and regimes, in order, on ONE handle -- and compares
every chunk list and every first[] bit for bit with the CPU oracle on the same
bytes (no tolerances).  tests/test_history_model.py shows, on the CPU, that in
every sequence an answer computed from the state of the call 1, 3 or 4 back
differs from the right one; a mismatch here names that call (harness.diagnose).

Engine state each sequence targets (chunkfs_amd/csrc/engine.hpp; small_ws_,
the staging blocks hb_, the device slots fs_, the workspace and d_gear_ are
FastEngine's, fast_engine.hpp; h_out_, the ring, d_data_ and the write windows
are HostPath's, host_path.hpp):

    S1  h_out_ (the host-mapped chunk list), the pinned ring, d_data_; on the
        default handle also small_ws_ and the feed words
    S2  the 4 ring slots, small_ws_ (device copy, block records, counts)
    S3  staging blocks (zero-copy stream tables), the 4 device slots and their
        `tables` caches, the workspace (grown, never shrunk), look-back
        descriptors, small_ws_
    S4  3 host staging blocks x 4 device slots under async bursts, `tables`
    S5  walk workspaces and flags, walk staging block, the 2 walk contexts
        and their threads, the Rabin tables
    S6  d_gear_ as seen by the small kernel, the pipeline, async batches and
        the write path
    S7  the write windows and the carried chunk, h_out_
    S8  the stream an async batch runs on vs the caller's stream
"""
import time

import numpy as np
import pytest

import history_harness as hh
import oracle

pytestmark = pytest.mark.gpu


def _handle(algo, sizes):
    import chunkfs_amd as c
    p = c.SizeParams(*sizes)
    if algo == "seq":
        return c.SeqChunker(c.OperationMode.Increasing, p)
    return {"fast": c.FastChunker, "rabin": c.RabinChunker, "ultra": c.UltraChunker, "leap": c.LeapChunker}[algo](p)


def _run(seq, ch):
    import torch
    t0 = time.perf_counter()
    n = hh.run(seq, ch, torch)
    print(f"{seq.name}: {n} results exact in {time.perf_counter() - t0:.2f} s")
    return n


@pytest.mark.parametrize("path", ["pipeline", "small"])
def test_s1_tails_after_3MiB_calls(monkeypatch, path):
    """S1, the recorded failing state: 3 MiB + 17 and 1 MiB calls, then the
    tails sweep shuffled and alternating between two buffers, on the scan +
    resolve pipeline (CHUNKFS_AMD_SMALL=0, where both red runs were) and on
    the default handle (one-launch small kernel).  The host guard of
    cdc_chunk_data must not have tripped: it may not hide a race here."""
    import chunkfs_amd as c
    if path == "pipeline":
        monkeypatch.setenv("CHUNKFS_AMD_SMALL", "0")
    seq = hh.s1()
    ch = _handle("fast", seq.sizes)
    _run(seq, ch)
    st = c.host_stats(ch)
    assert st["guard_trips"] == 0
    assert st["calls"] == len(seq.ops) - 1  # (the empty call returns before the engine)
    assert (st["small_calls"] == 0) if path == "pipeline" else (st["small_calls"] >= st["calls"])
    ch.close()


def test_s2_ring_slots_and_small_workspace():
    """S2: 13 one-launch calls on the default handle, every ring slot used
    three times or more with other bytes and other lengths, the golden vector
    that once lost three cuts among them (splitmix64, 1 048 909 bytes, min
    8192, 4 calls after 1 MiB + 909 other bytes in its slot)."""
    import chunkfs_amd as c
    seq = hh.s2()
    ch = c.FastChunker()
    assert (ch.sizes.min, ch.sizes.avg, ch.sizes.max) == seq.sizes
    _run(seq, ch)
    st = c.host_stats(ch)
    assert st["guard_trips"] == 0 and st["small_calls"] == len(seq.ops)
    ch.close()


def test_s3_regime_switching():
    """S3: small kernel, zero-copy tables, uploaded tables, pipeline, empty
    batches and n = 0 interleaved on one handle; the same pointers again in
    the same device slot with every length + 1, then with rewritten bytes; a
    40 MiB batch, then one span in the grown workspace."""
    seq = hh.s3()
    ch = _handle("fast", seq.sizes)
    _run(seq, ch)
    ch.close()


def test_s4_async_slot_reuse():
    """S4: two bursts of async batches of more than 8 MiB (10 ended by
    cdc_batch_sync, 9 by a host cdc_chunk_data): batch k - 3 has another
    stream count, batch k - 4 the same pointers and one length one byte
    shorter.  (tests/test_gpu_async.py covers the burst shapes and the drain
    rules; this adds the near-equal tables in one slot.)"""
    seq = hh.s4()
    ch = _handle("fast", seq.sizes)
    _run(seq, ch)
    assert ch.batch_sync() == 0
    ch.close()


@pytest.mark.parametrize("algo", hh.WALK_ALGOS)
def test_s5_walk_rules(algo):
    """S5: zero-copy, 65-stream, > 8 MiB synchronous and async batches, the
    first pointers again with length + 1, a quiet run and plain random bytes
    on one walk handle; Rabin changes its polynomial once the async contexts
    exist, and every later result -- the contexts' too -- is the oracle's
    with it."""
    seq = hh.s5(algo)
    ch = _handle(algo, seq.sizes)
    _run(seq, ch)
    ch.close()


def test_s6_gear_change_after_use():
    """S6: cdc_set_gear after the small kernel, the pipeline, an async burst
    and a finished streaming write have run: each path again, same bytes, new
    table."""
    seq = hh.s6()
    ch = _handle("fast", seq.sizes)
    _run(seq, ch)
    ch.close()


def test_s7_two_writes_one_handle():
    """S7: a write that crosses a 256 MiB window (a carried chunk), a host
    cdc_chunk_data, a second shorter write of other bytes."""
    import chunkfs_amd as c
    seq = hh.s7()
    ch = _handle("fast", seq.sizes)
    _run(seq, ch)
    assert c.host_stats(ch)["guard_trips"] == 0
    ch.close()


S8_BYTES = 10 * (1 << 20) + 64
S8_FILLS = 48  # 1 GiB fills queued ahead of the input's copy (~15 ms of device work)


@pytest.mark.parametrize("algo", ["fast"] + list(hh.WALK_ALGOS))
def test_s8_stream_order(algo):
    """S8: a batch reads its input after the work already on the caller's
    stream.  On a non-default stream: a long run of fills, then the copy that
    writes the input (zeros until then), then the submit with no host wait --
    the copy's event is still pending when the submit returns, so the input
    did not exist at submit time -- and the result is the oracle's on the
    copied bytes, not the chunking of zeros.  Async (FastCDC's scans run on
    that stream; a walk batch's context waits for an event recorded on it),
    then the synchronous call the same way."""
    import torch
    n = S8_BYTES
    src_np = oracle.splitmix64_bytes(n, 91)
    seq = hh.Sequence(f"S8-{algo}", algo, hh.FAST, {"B": src_np}, [hh.batch(("B", 0, n))])
    want = hh.model(seq)[0].ref
    zeros = hh.model(hh.Sequence("zeros", algo, hh.FAST, {"B": np.zeros(n, np.uint8)}, [hh.batch(("B", 0, n))]))[0].ref
    assert not hh.same_lists(want.lists, zeros.lists)
    ch = _handle(algo, hh.FAST)
    src = torch.from_numpy(src_np).to("cuda:0")
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:0")
    scratch = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")
    cap = ch.batch_max_chunks([n])
    out = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
    s = torch.cuda.Stream()
    args = ([buf.data_ptr()], [n], out.data_ptr(), cap)
    # Everything the measured calls use exists beforehand (the walk contexts,
    # the second stream, the workspaces: creating them synchronises the device).
    buf[:n].copy_(src)
    torch.cuda.synchronize()
    for _ in range(4):
        ch.chunk_batch_device_async(*args, stream=s.cuda_stream)
    ch.batch_sync()
    ch.chunk_batch_device(*args, stream=s.cuda_stream)
    for mode in ("async", "sync"):
        buf.zero_()
        out.zero_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            for k in range(S8_FILLS):
                scratch.fill_(k)
            buf[:n].copy_(src)
            e1.record()
        t0 = time.perf_counter()
        if mode == "async":
            first = ch.chunk_batch_device_async(*args, stream=s.cuda_stream)
            submit_ms = (time.perf_counter() - t0) * 1e3
            unwritten = not e1.query()
            ch.batch_sync()
        else:
            first = ch.chunk_batch_device(*args, stream=s.cuda_stream)
            submit_ms, unwritten = (time.perf_counter() - t0) * 1e3, None
        torch.cuda.synchronize()
        print(f"S8 {algo} {mode}: queued work {e0.elapsed_time(e1):.2f} ms, call returned after {submit_ms:.3f} ms, "
              f"input unwritten at return: {unwritten}")
        if mode == "async":
            assert unwritten, "the queue ahead of the input's copy was too short to prove anything: lengthen it"
        got = hh.Result([out[:int(first[1])].cpu().numpy().view(np.uint64).reshape(-1, 2)], first)
        where, _ = hh.first_difference(got, want)
        if where is not None:
            what = " (= the chunking of zeros: the input was read before it was written)" \
                if hh.same_lists(got.lists, zeros.lists) else ""
            pytest.fail(f"S8 {algo} {mode} on a caller's stream: {where[0]}: got {where[1]}, want {where[2]}{what}")
    ch.close()
