"""Call-sequence harness: results must not depend on what a handle ran before.

A Sequence is a script of ops run on ONE chunker handle, in order.  The
entry points:

    host(buf, n)            cdc_chunk_data on the host bytes buf[:n]
    batch(*streams)         cdc_chunk_batch_device
    submit(*streams)        cdc_chunk_batch_device_async (checked once drained)
    sync()                  cdc_batch_sync
    rewrite(buf, array)     new bytes at the same (device) address
    write(buf, n, seg)      cdc_fs_write (the streaming write path)
    gear(table), poly(p)    cdc_set_gear / cdc_set_rabin_poly

A stream is (buffer name, offset, length): buffers are named so that two ops
can use the same device pointers with other lengths or other bytes.

model(seq) walks the script with the CPU oracle alone (oracle.fastcdc /
oracle.cdc / oracle.fs_write on the same bytes, with the table or polynomial
in force at that op) and gives the expected answer of every result-producing
op (a "call").  run(seq, handle, torch) executes the script on the GPU and
compares every chunk list and every first[] bit for bit; a mismatch raises
with a message that diagnoses itself (diagnose): the op, the history before
it, the first differing entry, and whether that entry is what a state left by
the call 1, 3 or 4 calls earlier would give -- as that call's list entry
(the host read a result too early, or a slot was not rewritten) or as this
call's bytes cut with that call's lengths (the device used old tables).
Those distances are the previous call, the host staging blocks (3 in
rotation) and the device slots / ring slots (4).

power_violations(seq) is the condition on the inputs that makes the above
meaningful, checked on the CPU (tests/test_history_model.py): every call's
right answer differs from each of those stale answers.
"""
import functools

import numpy as np

import oracle

DISTANCES = (1, 3, 4)
MB = 1 << 20


# ---- script ---------------------------------------------------------------------

def host(buf, n):
    return ("host", ((buf, 0, int(n)),))


def batch(*streams):
    return ("batch", tuple((b, int(o), int(n)) for b, o, n in streams))


def submit(*streams):
    return ("async", tuple((b, int(o), int(n)) for b, o, n in streams))


def sync():
    return ("sync",)


def rewrite(buf, array):
    return ("rewrite", buf, np.ascontiguousarray(array, dtype=np.uint8))


def write(buf, n, seg=MB):
    return ("write", ((buf, 0, int(n)),), int(seg))


def gear(table):
    return ("gear", np.ascontiguousarray(table, dtype=np.uint64))


def poly(p):
    return ("poly", int(p))


CALLS = ("host", "batch", "async", "write")


class Sequence:
    """name, algorithm ("fast", "rabin", "ultra", "leap", "seq"), sizes, the
    named buffers' first contents and the ops.  `light`: op indices that leave
    the slot rotations alone (one-launch small calls, n = 0): the stale
    distances are also checked with those calls left out."""

    def __init__(self, name, algo, sizes, buffers, ops, light=()):
        self.name, self.algo, self.sizes = name, algo, tuple(sizes)
        self.buffers = {k: np.ascontiguousarray(v, dtype=np.uint8) for k, v in buffers.items()}
        self.ops = list(ops)
        self.light = frozenset(light)
        self._model = None


def describe(op):
    k = op[0]
    if k in CALLS:
        st = op[1]
        if len(st) > 4:
            body = f"{len(st)} streams, {sum(n for _, _, n in st)} B, first {st[0][0]}[{st[0][1]}:+{st[0][2]}]"
        else:
            body = ", ".join(f"{b}[{o}:+{n}]" for b, o, n in st) or "n=0"
        return f"{k}({body}{', seg=%d' % op[2] if k == 'write' else ''})"
    if k == "rewrite":
        return f"rewrite({op[1]}, {op[2].size} B)"
    if k == "gear":
        return "set_gear"
    if k == "poly":
        return f"set_poly({op[1]:#x})"
    return k


# ---- oracle model ---------------------------------------------------------------

class Result:
    """lists: one (k, 2) uint64 array of (offset, length) per stream (a write:
    its spans with their file offsets); first: first[n+1] of a batch, or None."""

    def __init__(self, lists, first=None):
        self.lists = [np.asarray(a, dtype=np.uint64).reshape(-1, 2) for a in lists]
        self.first = None if first is None else np.asarray(first, dtype=np.uint64).reshape(-1)


def _first_of(lists):
    return np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.uint64)


def spans_to_pairs(lengths):
    ln = np.asarray(lengths, dtype=np.uint64).reshape(-1)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64) if ln.size else ln
    return np.stack([off, ln], axis=1)


class Call:
    """One result-producing op with everything its answer depends on."""

    def __init__(self, seq, index, op, arrays, table, rabin_poly):
        self.seq, self.index, self.op, self.kind = seq, index, op, op[0]
        self.streams = op[1]
        self.arrays = arrays          # the streams' buffers as they were at this op
        self.table, self.rabin_poly = table, rabin_poly
        self.seg = op[2] if self.kind == "write" else None
        self.ref = Result(self.cut(), None)
        if self.kind in ("batch", "async"):
            self.ref.first = _first_of(self.ref.lists)

    def cut_one(self, k, n=None):
        """The oracle's chunks of stream k, or of its first n bytes (n may
        exceed the op's length, up to the buffer's end)."""
        _, off, own = self.streams[k]
        n = own if n is None else n
        data = self.arrays[k][off:off + n]
        s = self.seq
        if self.kind == "write":
            ln, _ = oracle.fs_write(s.algo, data, *s.sizes, seg_size=self.seg, gear=self.table)
            return spans_to_pairs(ln)
        if data.size == 0:
            return np.zeros((0, 2), np.uint64)
        if s.algo == "fast":
            return oracle.fastcdc(data, *s.sizes, gear=self.table)
        return oracle.cdc(s.algo, data, *s.sizes, rabin_poly=self.rabin_poly)

    def cut(self, lens=None):
        return [self.cut_one(k, None if lens is None else lens[k]) for k in range(len(self.streams))]

    def with_lengths_of(self, other):
        """This call's bytes cut with `other`'s lengths, stream by stream (a
        length past the buffer's end is clipped); None when no length differs."""
        lens, differs = [], False
        for k, (_, off, n) in enumerate(self.streams):
            m = other.streams[k][2] if k < len(other.streams) else n
            m = min(m, self.arrays[k].size - off)
            differs |= m != n
            lens.append(m)
        return self.cut(lens) if differs else None


def model(seq):
    """The calls of `seq`, each with its oracle answer (computed once)."""
    if seq._model is None:
        bufs = dict(seq.buffers)
        table, rp, calls = None, None, []
        for i, op in enumerate(seq.ops):
            if op[0] in CALLS:
                for b, off, n in op[1]:
                    assert off + n <= bufs[b].size, (seq.name, i, b)
                calls.append(Call(seq, i, op, [bufs[b] for b, _, _ in op[1]], table, rp))
            elif op[0] == "rewrite":
                assert op[2].size <= bufs[op[1]].size
                new = bufs[op[1]].copy()  # (earlier calls keep the array they saw)
                new[:op[2].size] = op[2]
                bufs[op[1]] = new
            elif op[0] == "gear":
                table = op[1]
            elif op[0] == "poly":
                rp = op[1]
        seq._model = calls
    return seq._model


def same_lists(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def first_difference(got, ref):
    """None, or (where, got entry, wanted entry) of the first differing entry."""
    if len(got.lists) != len(ref.lists):
        return (f"stream count {len(got.lists)} vs {len(ref.lists)}", None, None), None
    for s, (g, r) in enumerate(zip(got.lists, ref.lists)):
        n = min(len(g), len(r))
        bad = np.nonzero((g[:n] != r[:n]).any(axis=1))[0]
        k = int(bad[0]) if bad.size else (n if len(g) != len(r) else None)
        if k is not None:
            return (f"stream {s} entry {k} ({len(g)} vs {len(r)} chunks)",
                    g[k].tolist() if k < len(g) else None, r[k].tolist() if k < len(r) else None), (s, k)
    if ref.first is not None:
        gf = got.first if got.first is not None else np.zeros(0, np.uint64)
        if gf.shape != ref.first.shape or (gf != ref.first).any():
            return (f"first[] {gf.tolist()[:8]} vs {ref.first.tolist()[:8]}", None, None), None
    return None, None


def _spaces(seq, calls):
    """Index spaces the stale distances are counted in: every call, and the
    calls that rotate the slots (seq.light left out)."""
    every = list(range(len(calls)))
    heavy = [c for c in every if calls[c].index not in seq.light]
    return [every] if heavy == every else [every, heavy]


def stale_candidates(seq, calls, ci):
    """(distance, earlier call) pairs a stale state of call ci could stem from."""
    out = []
    for space in _spaces(seq, calls):
        if ci not in space:
            continue
        p = space.index(ci)
        for d in DISTANCES:
            if p - d >= 0 and (d, space[p - d]) not in out:
                out.append((d, space[p - d]))
    return out


def diagnose(seq, ci, got):
    """The mismatch message of call ci (None when `got` is right)."""
    calls = model(seq)
    c = calls[ci]
    where, at = first_difference(got, c.ref)
    if where is None:
        return None
    lines = [f"{seq.name} ({seq.algo} {seq.sizes}): op {c.index} {describe(c.op)} is wrong",
             f"  first difference: {where[0]}: got {where[1]}, want {where[2]}",
             "  history (last 12 ops): " + "; ".join(f"{i} {describe(o)}"
                                                      for i, o in list(enumerate(seq.ops[:c.index]))[-12:])]
    found = False
    for d, cj in stale_candidates(seq, calls, ci):
        j = calls[cj]
        if same_lists(got.lists, j.ref.lists):
            lines.append(f"  = the WHOLE answer of op {j.index} {describe(j.op)} ({d} calls back)")
            found = True
        if at is None or where[1] is None:
            continue
        s, k = at
        if s < len(j.ref.lists) and k < len(j.ref.lists[s]) and j.ref.lists[s][k].tolist() == where[1]:
            lines.append(f"  that entry = op {j.index}'s list entry ({d} calls back: a stale chunk list)")
            found = True
        alt = c.with_lengths_of(j)
        if alt is not None and k < len(alt[s]) and alt[s][k].tolist() == where[1]:
            lines.append(f"  that entry = this op's bytes cut with op {j.index}'s length {j.streams[s][2] if s < len(j.streams) else None} "
                         f"({d} calls back: a stale length)")
            found = True
    if not found:
        lines.append("  that entry is neither the list entry nor the length of the calls 1, 3 or 4 back")
    return "\n".join(lines)


def power_violations(seq):
    """Every way an answer computed from the state of the call 1, 3 or 4 back
    would go unseen: [] when the script can tell them all apart."""
    calls = model(seq)
    bad = []
    for ci, c in enumerate(calls):
        for d, cj in stale_candidates(seq, calls, ci):
            j = calls[cj]
            if same_lists(c.ref.lists, j.ref.lists):
                bad.append(f"{seq.name}: op {c.index} {describe(c.op)} has the answer of op {j.index} ({d} back)")
            alt = c.with_lengths_of(j)
            if alt is not None and same_lists(alt, c.ref.lists):
                bad.append(f"{seq.name}: op {c.index} {describe(c.op)} cut with op {j.index}'s lengths ({d} back) "
                           "gives its own answer")
    return bad


# ---- GPU runner -----------------------------------------------------------------

def run(seq, handle, torch):
    """Execute seq.ops on `handle`; AssertionError with diagnose()'s message at
    the first wrong result.  Returns the number of results compared."""
    import chunkfs_amd as c
    calls = model(seq)
    by_op = {cl.index: ci for ci, cl in enumerate(calls)}
    dev, host_now = {}, dict(seq.buffers)
    for name, a in seq.buffers.items():
        t = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda:0")
        t[:a.size] = torch.from_numpy(a).to("cuda:0")
        dev[name] = t
    torch.cuda.synchronize()
    pending, checked = [], 0

    def collect(out, first, n):
        first = np.asarray(first, dtype=np.uint64)
        total = int(first[n]) if first.size == n + 1 else 0
        rows = out[:min(total, out.shape[0])].cpu().numpy().view(np.uint64).reshape(-1, 2)
        lists = [rows[int(first[i]):int(first[i + 1])] for i in range(n)]
        return Result(lists, first)

    def check(ci, got):
        nonlocal checked
        msg = diagnose(seq, ci, got)
        if msg:
            raise AssertionError(msg)
        checked += 1

    def drain():
        while pending:
            ci, out, first, n = pending.pop(0)
            check(ci, collect(out, first, n))

    for i, op in enumerate(seq.ops):
        k = op[0]
        if k == "host":
            b, off, n = op[1][0]
            got = handle.chunk_array(host_now[b][off:off + n]).copy()
            drain()  # (the call completed the batches in flight first)
            check(by_op[i], Result([got]))
        elif k in ("batch", "async"):
            ptrs = [dev[b].data_ptr() + off for b, off, _ in op[1]]
            lens = [n for _, _, n in op[1]]
            cap = handle.batch_max_chunks(lens)
            out = torch.empty((max(cap, 1), 2), dtype=torch.int64, device="cuda:0")
            if k == "async":
                first = handle.chunk_batch_device_async(ptrs, lens, out.data_ptr(), cap)
                pending.append((by_op[i], out, first, len(lens)))
            else:
                first = handle.chunk_batch_device(ptrs, lens, out.data_ptr(), cap)
                drain()
                check(by_op[i], collect(out, first, len(lens)))
        elif k == "sync":
            assert handle.batch_sync() >= 0
            drain()
        elif k == "rewrite":
            assert not pending, "rewrite with batches in flight"
            new = host_now[op[1]].copy()
            new[:op[2].size] = op[2]
            host_now[op[1]] = new
            dev[op[1]][:op[2].size] = torch.from_numpy(op[2]).to("cuda:0")
            torch.cuda.synchronize()
        elif k == "write":
            assert not pending, "write with batches in flight"
            b, off, n = op[1][0]
            spans, _ = c.write_spans(handle, host_now[b][off:off + n], op[2])
            check(by_op[i], Result([spans_to_pairs(spans)]))
        elif k == "gear":
            handle.set_gear(op[1])
        elif k == "poly":
            handle.set_poly(op[1])
        else:
            raise ValueError(k)
    assert not pending, "the script ends with batches in flight (add sync())"
    assert checked == len(calls)
    return checked


# ---- the scripted sequences -------------------------------------------------------

FAST = (4096, 8192, 16384)
DEFAULT = (8192, 16384, 65536)      # FastChunker's default sizes
WALK_ALGOS = ("rabin", "ultra", "leap", "seq")
BLOCK = 32 << 10                    # the small kernel's block of input
RING_SLOTS = 4
GOLDEN = ("splitmix64", 1048909, 9)  # the golden vector that once lost three cuts (min 8192)
SECOND_GEAR_SEED = 0xBEEF
SECOND_POLY = 0x2E8A2B1C4F0B35

rnd = oracle.splitmix64_bytes


def tails_lengths():
    """test_tails_of_every_length's lengths (tests/test_gpu_parity.py)."""
    return list(range(0, 200)) + list(range(4000, 4200)) + list(range(8100, 8300)) + \
        list(range(16300, 16500)) + list(range(2 * 16384 - 100, 2 * 16384 + 2))


@functools.lru_cache(maxsize=None)
def s1():
    """S1: the recorded failing state of the host path.  Two calls of
    3 MiB + 17 and 1 MiB (test_random_streams_bit_exact's), then the tails
    sweep in a fixed shuffled order, alternating between base buffers A and B
    whose first cuts differ: the previous call's answer -- the wrong value of
    both red runs -- is another buffer's cuts at another length."""
    n0, n1 = 3 * MB + 17, MB
    bufs = {"R0": rnd(n0, 31 + n0), "R1": rnd(n1, 31 + n1),
            "A": rnd(2 * 16384 + 64, 77), "B": rnd(2 * 16384 + 64, 78)}
    lens = np.array(tails_lengths())[np.random.default_rng(20240607).permutation(len(tails_lengths()))]
    ops = [host("R0", n0), host("R1", n1)] + [host("AB"[i & 1], int(n)) for i, n in enumerate(lens)]
    return Sequence("S1", "fast", FAST, bufs, ops)


S2_LENGTHS = (MB + 909, 3 * MB, 40000, 4 * MB, 1, 8192)
S2_GOLDEN_AT = 4   # the call 4 back (same ring slot) was 1 MiB + 909 bytes of other content
# picked until stale_block_violations() is empty for every call (tests/test_history_model.py)
S2_SEEDS = (5170, 5020, 5031, 5016, 4104, 4105, 4106, 4107, 5171, 4109, 4110, 4111)


@functools.lru_cache(maxsize=None)
def s2():
    """S2: ring slots and the small kernel's workspace (default handle, host
    path): 13 one-launch calls, every ring slot used three times or more, each
    call with other bytes, lengths cycling long / short so that a slot's (and
    the device copy's) earlier, longer content still lies beyond the new
    length; the golden vector that once lost three cuts runs 4 calls after
    1 MiB + 909 other bytes in its slot."""
    bufs, ops = {}, []
    for i, seed in enumerate(S2_SEEDS):
        n = S2_LENGTHS[i % len(S2_LENGTHS)]
        bufs[f"H{i}"] = rnd(n, seed)
        ops.append(host(f"H{i}", n))
    bufs["G"] = rnd(GOLDEN[1], GOLDEN[2])
    ops.insert(S2_GOLDEN_AT, host("G", GOLDEN[1]))
    return Sequence("S2", "fast", DEFAULT, bufs, ops)


def stale_block_violations(seq, every, only=None):
    """S2's condition on the bytes: for each call and each 32 KiB block of it,
    the answer changes when that block still holds what the memory held before
    the call -- `every` = 1: one buffer rewritten by every call (the small
    kernel's device copy), RING_SLOTS: the ring slot, rewritten by every 4th.
    Only bytes the cut rule reads can matter: FastCDC skips the first `min`
    bytes of every chunk, so a block's stale bytes are taken where an earlier
    call wrote them AND the rule reads them; a block with no such byte is left
    out (a buffer no longer than `min` has none: its length is what a stale
    state would get wrong, power_violations).  Returns the violations and the
    number of blocks checked."""
    calls = model(seq)
    sizes, bad, blocks = seq.sizes, [], 0
    skip = (sizes[0] // 2) * 2
    for ci, c in enumerate(calls):
        if only is not None and ci != only:
            continue
        _, _, n = c.streams[0]
        data = c.arrays[0][:n]
        image, written = np.zeros(max(cl.streams[0][2] for cl in calls), np.uint8), 0
        for cj in range(ci % every, ci, every):
            m = calls[cj].streams[0][2]
            image[:m] = calls[cj].arrays[0][:m]
            written = max(written, m)
        read = np.zeros(n, bool)
        for o, ln in c.ref.lists[0].astype(np.int64):
            read[o + skip:o + ln + 1] = True
        read[written:] = False
        starts = c.ref.lists[0][:, 0].astype(np.int64)
        for lo in range(0, n, BLOCK):
            hi = min(lo + BLOCK, n)
            if not read[lo:hi].any():
                continue
            blocks += 1
            # cut again from the chunk that holds the block's first byte (every
            # chunk starts afresh), a few maximum chunks past the block
            a = int(starts[np.searchsorted(starts, lo, side="right") - 1])
            z = min(n, hi + 4 * sizes[2])
            mod = data[a:z].copy()
            mod[lo - a:hi - a][read[lo:hi]] = image[lo:hi][read[lo:hi]]
            if same_lists([oracle.fastcdc(mod, *sizes)], [oracle.fastcdc(data[a:z], *sizes)]):
                bad.append(f"{seq.name}: op {c.index} block {lo // BLOCK}: stale bytes (rewritten every {every}) move no cut")
    return bad, blocks


def _m65():
    """65 streams in one buffer: 48 KiB apart, 20000 + 371 k bytes."""
    return [("M", 49152 * k, 20000 + 371 * k) for k in range(65)]


def _plus1(streams):
    return [(b, o, n + 1) for b, o, n in streams]


@functools.lru_cache(maxsize=None)
def s3():
    """S3: regime switching on one FastCDC handle (device batches): the
    one-launch small kernel (one stream <= 4 MiB), zero-copy stream tables
    read from the pinned staging blocks (3 streams <= 8 MiB), uploaded tables
    (65 streams), the pipeline (9 MiB + 5), an all-empty batch and n = 0, each
    twice or more, interleaved.  The batches that go through a submit are
    laid out four apart, so each device slot's `tables` cache sees the same
    pointers again: with every length + 1 (the cache has to notice), then
    with the same lengths and rewritten bytes (a hit must still follow the
    bytes).  Then a 40 MiB batch grows the workspace and a one-span batch runs
    in it with the big batch's counts beyond total_spans."""
    q = [("Q0", 0, MB + 3), ("Q1", 0, 700001), ("Q2", 0, 300017)]
    p, lg = [("P", 0, MB + MB // 2 + 11)], [("L", 0, 9 * MB + 5)]
    m = _m65()
    bufs = {"Q0": rnd(MB + 64, 31), "Q1": rnd(700064, 32), "Q2": rnd(300064, 33), "P": rnd(2 * MB, 34),
            "M": rnd(65 * 49152, 35), "L": rnd(9 * MB + 64, 36), "G": rnd(40 * MB, 37), "X": rnd(8192, 38)}
    empty3 = [("Q0", 0, 0), ("Q1", 0, 0), ("Q2", 0, 0)]
    empty2 = [("Q0", 0, 0), ("L", 0, 0)]
    big = [("G", 10 * MB * k, 10 * MB - 16 * k) for k in range(4)]
    ops = [
        batch(*p),            # 0  small kernel
        batch(*q),            # 1  submit 0: zero-copy tables
        batch(*m),            # 2  submit 1: uploaded tables
        batch(),              # 3  n = 0
        batch(*lg),           # 4  submit 2: pipeline
        batch(*empty3),       # 5  submit 3: all empty
        batch(*_plus1(q)),    # 6  submit 4
        batch(*_plus1(m)),    # 7  submit 5: slot 1 again, every length + 1
        batch(*_plus1(p)),    # 8  small kernel
        batch(*_plus1(lg)),   # 9  submit 6: slot 2 again, length + 1
        batch(*empty2),       # 10 submit 7
        rewrite("Q0", rnd(MB + 64, 41)), rewrite("Q1", rnd(700064, 42)), rewrite("Q2", rnd(300064, 43)),
        rewrite("P", rnd(2 * MB, 44)), rewrite("M", rnd(65 * 49152, 45)), rewrite("L", rnd(9 * MB + 64, 46)),
        batch(*_plus1(q)),    # 17 submit 8: same pointers and lengths, other bytes
        batch(*_plus1(m)),    # 18 submit 9: slot 1, a cache hit
        batch(),              # 19 n = 0
        batch(*_plus1(lg)),   # 20 submit 10: slot 2, a cache hit
        batch(*_plus1(p)),    # 21 small kernel, other bytes
        batch(*q),            # 22 submit 11
        batch(*big),          # 23 submit 12: grows the workspace
        batch(("X", 0, 5000), ("X", 0, 0)),  # 24 submit 13: one span in the grown workspace
        batch(*lg),           # 25 submit 14: pipeline after the regrowth
        batch(*m),            # 26 submit 15
    ]
    return Sequence("S3", "fast", FAST, bufs, ops, light=(0, 3, 8, 19, 21))


def _s4_batch(k):
    """Async batch k: one stream (even k) or two (odd k), more than 8 MiB;
    batch k - 4 has the same pointers and one length one byte shorter."""
    bump = k // 4 + 16 * ((k % 4) // 2)
    if k % 2 == 0:
        return [("U", 0, 9 * MB + 5 + bump)]
    return [("V", 0, 5 * MB + 3 + bump), ("W", 0, 4 * MB + MB // 2)]


@functools.lru_cache(maxsize=None)
def s4():
    """S4: async FastCDC slot reuse: bursts of batches of more than 8 MiB, in
    flight three at a time -- host staging block k % 3, device slot k % 4.
    Batch k - 3 (the block's last user) has another stream count; batch k - 4
    (the slot's, whose uploaded tables are cached) has the same pointers and
    one length one byte shorter.  One burst of 10 ends with cdc_batch_sync,
    one of 9 with a host cdc_chunk_data, which drains implicitly."""
    bufs = {"U": rnd(9 * MB + 128, 51), "V": rnd(5 * MB + 128, 52), "W": rnd(4 * MB + MB // 2 + 64, 53),
            "H": rnd(300001, 54)}
    ops = [submit(*_s4_batch(k)) for k in range(10)] + [sync()]
    ops += [submit(*_s4_batch(k)) for k in range(10, 19)] + [host("H", 300001), sync()]
    return Sequence("S4", "fast", FAST, bufs, ops)


@functools.lru_cache(maxsize=None)
def s5(algo):
    """S5: one segment-walk handle (Rabin / Ultra / Leap / Seq) through its
    states: zero-copy tables in the staging block, a 65-stream batch
    (uploaded tables), a synchronous batch of more than 8 MiB (grown walk
    workspace), two async batches (one per walk context), the first batch's
    pointers again with every length + 1, an input with a quiet run, a plain
    random one, and two more async batches on the contexts.  Rabin installs
    another polynomial once the contexts exist: every later result, the
    contexts' too, is the oracle's with that polynomial."""
    q = [("Q0", 0, MB + 3), ("Q1", 0, 700001), ("Q2", 0, 300017)]
    quiet = rnd(2 * MB, 66)
    quiet[700001:700001 + 600000] = 0
    bufs = {"Q0": rnd(MB + 64, 61), "Q1": rnd(700064, 62), "Q2": rnd(300064, 63), "M": rnd(65 * 49152, 64),
            "L": rnd(9 * MB + 64, 65), "Z": quiet, "R": rnd(MB + 77, 67), "K": rnd(5 * MB, 68),
            "J": rnd(4 * MB, 69)}
    two = [("K", 0, 5 * MB - 7), ("J", 0, 4 * MB - 1)]
    ops = [batch(*q), batch(*_m65()), batch(("L", 0, 9 * MB + 5)),
           submit(("L", 0, 9 * MB + 21)), submit(*two), sync()]
    if algo == "rabin":
        ops.append(poly(SECOND_POLY))
    ops += [batch(*_plus1(q)), batch(("Z", 0, 2 * MB)), batch(("R", 0, MB + 77)),
            submit(*_plus1(two)), submit(("L", 0, 9 * MB + 37)), sync()]
    return Sequence(f"S5-{algo}", algo, FAST, bufs, ops)


def second_gear():
    return rnd(256 * 8, SECOND_GEAR_SEED).view(np.uint64).copy()


@functools.lru_cache(maxsize=None)
def s6():
    """S6: cdc_set_gear after the handle has served the small kernel, the
    pipeline, an async burst and a finished streaming write: the next call on
    each of those paths, on the same bytes as before, is the oracle's with the
    new table (the device table d_gear_ is shared by all of them)."""
    bufs = {"S": rnd(MB + 17, 71), "L": rnd(9 * MB + 64, 72), "W": rnd(3 * MB + 99, 73)}
    burst = [submit(("L", 0, 9 * MB + 6 + k)) for k in range(3)] + [sync()]
    serve = [host("S", MB + 17), batch(("L", 0, 9 * MB + 5))] + burst + [write("W", 3 * MB + 99)]
    return Sequence("S6", "fast", FAST, bufs, serve + [gear(second_gear())] + serve)


S7_FIRST = (256 << 20) + MB + 4321


@functools.lru_cache(maxsize=None)
def s7():
    """S7: the write path's state across writes: a first cdc_fs_write that
    crosses a 256 MiB device window (a carried chunk left in the other
    window), a host cdc_chunk_data (the same host-mapped chunk list h_out_),
    then a second, shorter write of other bytes."""
    bufs = {"W1": rnd(S7_FIRST, 81), "H": rnd(300001, 82), "W2": rnd(3 * MB + 99, 83)}
    return Sequence("S7", "fast", FAST, bufs, [write("W1", S7_FIRST), host("H", 300001), write("W2", 3 * MB + 99)])


NAMES = ["S1", "S2", "S3", "S4"] + [f"S5-{a}" for a in WALK_ALGOS] + ["S6", "S7"]


def get(name):
    """The sequence of that name (built on first use, then shared)."""
    if name.startswith("S5-"):
        return s5(name[3:])
    return {"S1": s1, "S2": s2, "S3": s3, "S4": s4, "S6": s6, "S7": s7}[name]()
