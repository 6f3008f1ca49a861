"""Async batches of the segment-walk algorithms (-m gpu): cdc_chunk_batch_device_async
on Rabin / UltraCDC / LeapCDC / SeqCDC / AE handles runs alternate batches on two
contexts (WalkEngine::submit), each on its own stream and host worker thread.
Every batch bit-exact vs the CPU oracle, whatever its context, and the drain
semantics those of the FastCDC pipeline (batch_sync, implicit drains)."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ALGOS = ["rabin", "ultra", "leap", "seq"]
SIZES = (4096, 8192, 16384)


def make(algo, sizes=SIZES):
    import chunkfs_amd as c
    cls = {"rabin": c.RabinChunker, "ultra": c.UltraChunker, "leap": c.LeapChunker}.get(algo)
    p = c.SizeParams(*sizes)
    return cls(p) if cls else c.SeqChunker(c.OperationMode.Increasing, p)


def _dev(torch, n, seed):
    a = oracle.splitmix64_bytes(n, seed)
    b = torch.empty(max(n, 16), dtype=torch.uint8, device="cuda:0")
    b[:n] = torch.from_numpy(a).to("cuda:0")
    return b, a


def _check(algo, out, first, arrays, sizes=SIZES):
    got = out.cpu().numpy().view(np.uint64)
    for i, a in enumerate(arrays):
        ref = oracle.cdc(algo, a, *sizes)
        seg = got[int(first[i]):int(first[i + 1])]
        assert seg.shape == ref.shape and (seg == ref).all(), f"{algo} stream {i} len={len(a)}"


@pytest.mark.parametrize("algo", ALGOS)
def test_walk_async_burst(algo):
    """Six back-to-back batches of varying shape (every context reused),
    results checked after one batch_sync."""
    import torch
    ch = make(algo)
    lens_all = [(12 << 20) + 5, 9 << 20, (5 << 20) + 999, 0, (10 << 20) + 64]
    data = [_dev(torch, n, 900 + i) for i, n in enumerate(lens_all)]
    shapes = [[0], [1, 2], [4, 3], [2, 0, 1], [1], [4, 2]]
    res = []
    for idx in shapes:
        lens = [lens_all[i] for i in idx]
        cap = ch.batch_max_chunks(lens)
        out = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
        first = ch.chunk_batch_device_async([data[i][0].data_ptr() for i in idx], lens, out.data_ptr(), cap)
        res.append((idx, out, first))
    assert ch.batch_sync() == int(res[-1][2][-1])
    assert ch.batch_sync() == 0
    for idx, out, first in res:
        _check(algo, out, first, [data[i][1] for i in idx])
    ch.close()


@pytest.mark.parametrize("algo", ["rabin", "seq"])
def test_walk_async_implicit_drain(algo):
    """A synchronous call on the handle completes the async batches first;
    the next batch_sync returns what that drain collected."""
    import torch
    ch = make(algo)
    b, a = _dev(torch, 11 << 20, 31)
    cap = ch.batch_max_chunks([len(a)])
    outs = [torch.empty((cap, 2), dtype=torch.int64, device="cuda:0") for _ in range(3)]
    firsts = [ch.chunk_batch_device_async([b.data_ptr()], [len(a)], o.data_ptr(), cap) for o in outs]
    small = oracle.splitmix64_bytes(300_000, 5)
    got = ch.chunk_array(small)  # (drains the three batches first)
    ref_small = oracle.cdc(algo, small, *SIZES)
    assert got.shape == ref_small.shape and (got.view(np.uint64) == ref_small).all()
    ref = oracle.cdc(algo, a, *SIZES)
    assert ch.batch_sync() == len(ref)
    for o, f in zip(outs, firsts):
        _check(algo, o, f, [a])
    ch.close()


def test_walk_async_off_equals_on(monkeypatch):
    """CHUNKFS_AMD_WALK_ASYNC=0 (batches complete inside the call) gives the
    same chunks."""
    import torch
    b, a = _dev(torch, 13 << 20, 77)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("CHUNKFS_AMD_WALK_ASYNC", mode)
        ch = make("ultra")
        cap = ch.batch_max_chunks([len(a)])
        o = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
        f = ch.chunk_batch_device_async([b.data_ptr()], [len(a)], o.data_ptr(), cap)
        got = ch.batch_sync()
        n = int(f[-1])
        assert got == (n if mode == "1" else 0)  # (off: the batch completed inside the call)
        outs[mode] = o[:n].cpu().numpy()
        ch.close()
    assert (outs["1"] == outs["0"]).all()


def test_walk_async_rabin_poly_applies():
    """A polynomial set on the handle reaches the async contexts."""
    import torch
    ch = make("rabin")
    poly = 0x3DA3358B4DC173
    ch.set_poly(poly)
    b, a = _dev(torch, 10 << 20, 12)
    cap = ch.batch_max_chunks([len(a)])
    o = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
    ch.chunk_batch_device_async([b.data_ptr()], [len(a)], o.data_ptr(), cap)
    n = ch.batch_sync()
    sync = make("rabin")
    sync.set_poly(poly)
    ref = sync.chunk_array(a)
    assert n == len(ref) and (o[:n].cpu().numpy().view(np.uint64) == ref.view(np.uint64)).all()
    ch.close()
    sync.close()


# ---- the contexts are WalkEngines of the handle's configuration ------------

def _submit(ch, torch, ptrs, lens):
    """One async batch with an output buffer of its own: (out, first)."""
    cap = ch.batch_max_chunks(lens)
    out = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
    return out, ch.chunk_batch_device_async(ptrs, lens, out.data_ptr(), cap)


def _same(out, first, refs):
    """Stream i's chunks out[first[i]:first[i+1]] equal refs[i], for every i."""
    got = out.cpu().numpy().view(np.uint64)
    assert int(first[0]) == 0 and len(first) == len(refs) + 1
    for i, ref in enumerate(refs):
        seg = got[int(first[i]):int(first[i + 1])]
        assert seg.shape == ref.shape and (seg == ref).all(), f"stream {i}"


def _seq_configured(c, p):
    return c.SeqChunker(c.OperationMode.Decreasing, p, c.SeqConfig(seq_length=7, jump_trigger=30, jump_size=128))


def _ae_configured(c, p):
    return c.AeChunker(p, window=3000, mode=c.AeMode.Min)  # (the default window for avg 8192 is 4767)


def _ae_ref(a, **kw):
    import ae_model
    return ae_model.chunk_array(a, *SIZES, **kw)


CONFIGURED = {
    "seq": (_seq_configured, lambda a: oracle.cdc("seq", a, *SIZES, seqcfg=(1, 7, 30, 128)),
            lambda a: oracle.cdc("seq", a, *SIZES)),
    "ae": (_ae_configured, lambda a: _ae_ref(a, w=3000, mode=1), _ae_ref),
}


@pytest.mark.parametrize("rule", sorted(CONFIGURED))
def test_walk_async_rule_configuration_reaches_contexts(rule):
    """A non-default SeqCDC / AE configuration: four async batches (two per
    context), each the oracle's with that configuration and none the default
    configuration's."""
    import torch
    import chunkfs_amd as c
    new, ref_of, default_of = CONFIGURED[rule]
    ch = new(c, c.SizeParams(*SIZES))
    data = [_dev(torch, n, 40 + i) for i, n in enumerate([(9 << 20) + 11, 10 << 20])]
    refs = [ref_of(a) for _, a in data]
    for (_, a), ref in zip(data, refs):
        d = default_of(a)
        assert d.shape != ref.shape or (d != ref).any()  # (a context on the defaults would show)
    order = [0, 1, 1, 0]  # (contexts 0 1 0 1: each chunks both buffers)
    res = [_submit(ch, torch, [data[i][0].data_ptr()], [len(data[i][1])]) for i in order]
    assert ch.batch_sync() == len(refs[order[-1]])
    for i, (out, first) in zip(order, res):
        _same(out, first, [refs[i]])
    ch.close()


@pytest.mark.parametrize("algo", ["rabin", "leap"])
def test_walk_async_context_workspace_regrows(algo):
    """Each context's workspace, stream tables and pinned block grow between
    its own batches: 1 x 9 MiB, 70 streams (table upload, two of them empty)
    of 12 MiB in all, 1 x 13 MiB, then the first pointers again with length +
    1; every shape twice in a row, so both contexts see it."""
    import torch
    ch = make(algo)
    b9, a9 = _dev(torch, (9 << 20) + 16, 61)
    b12, a12 = _dev(torch, 12 << 20, 62)
    b13, a13 = _dev(torch, 13 << 20, 63)
    piece, n9 = 185040, 9 << 20  # (a multiple of 16: every stream pointer stays aligned)
    cuts = [(k * piece, piece) for k in range(67)] + [(67 * piece, (12 << 20) - 67 * piece)]
    many = cuts[:5] + [None] + cuts[5:] + [None]  # None: an empty stream
    assert len(many) == 70 and sum(ln for _, ln in cuts) == 12 << 20
    shapes = [
        ([b9.data_ptr()], [n9], [a9[:n9]]),
        ([b12.data_ptr() + m[0] if m else 0 for m in many], [m[1] if m else 0 for m in many],
         [a12[m[0]:m[0] + m[1]] if m else a12[:0] for m in many]),
        ([b13.data_ptr()], [len(a13)], [a13]),
        ([b9.data_ptr()], [n9 + 1], [a9[:n9 + 1]]),
    ]
    res = []
    for ptrs, lens, arrays in shapes:
        refs = [oracle.cdc(algo, a, *SIZES) for a in arrays]
        res += [(_submit(ch, torch, ptrs, lens), refs) for _ in range(2)]
    assert ch.batch_sync() == sum(len(r) for r in res[-1][1])
    for (out, first), refs in res:
        _same(out, first, refs)
    ch.close()


def test_walk_async_handle_destroyed_with_batches_in_flight():
    """cdc_destroy without a batch_sync completes the enqueued batches; a
    fresh handle of the same rule then chunks as ever."""
    import torch
    ch = make("ultra")
    data = [_dev(torch, n, 70 + i) for i, n in enumerate([9 << 20, (10 << 20) + 48, (9 << 20) + 5])]
    res = [_submit(ch, torch, [b.data_ptr()], [len(a)]) for b, a in data]
    ch.close()
    for (out, first), (_, a) in zip(res, data):
        _same(out, first, [oracle.cdc("ultra", a, *SIZES)])
    ch = make("ultra")
    b, a = data[1]
    cap = ch.batch_max_chunks([len(a)])
    out = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
    _same(out, ch.chunk_batch_device([b.data_ptr()], [len(a)], out.data_ptr(), cap), [oracle.cdc("ultra", a, *SIZES)])
    ch.close()


def test_walk_async_and_sync_share_nothing_stale():
    """Async batch, a new polynomial, async batch, a 1 MiB synchronous call
    (zero-copy tables), batch_sync: each result is the oracle's with the
    polynomial in force at its submit, and batch_sync returns what the
    synchronous call's implicit drain collected."""
    import torch
    second = 0x2E8A2B1C4F0B35
    ch = make("rabin")
    b, a = _dev(torch, (10 << 20) + 32, 81)
    r1 = _submit(ch, torch, [b.data_ptr()], [len(a)])
    ch.set_poly(second)
    r2 = _submit(ch, torch, [b.data_ptr()], [len(a)])
    small = 1 << 20
    cap = ch.batch_max_chunks([small])
    out = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
    first = ch.chunk_batch_device([b.data_ptr()], [small], out.data_ptr(), cap)
    ref2 = oracle.cdc("rabin", a, *SIZES, rabin_poly=second)
    assert ch.batch_sync() == len(ref2)
    assert ch.batch_sync() == 0
    _same(*r1, [oracle.cdc("rabin", a, *SIZES)])
    _same(*r2, [ref2])
    _same(out, first, [oracle.cdc("rabin", a[:small], *SIZES, rabin_poly=second)])
    ch.close()
