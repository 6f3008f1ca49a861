"""FastCDC size table and a plain-Python model of the engine's derived
parameters (a helper of test_fast_sizes_model.py and test_gpu_fast_sizes.py).

The model restates, from the size triple alone, what FastEngine::create
(chunkfs_amd/csrc/fast_engine.cpp) derives: the mask pair, the candidate-test form,
the span size, the record cap, the chunk starts per span and the one-launch
small kernel's eligibility.  The GPU tests compare the two values the engine
exports (cdc_debug_record_cap, the span count of cdc_debug_copy) with it, so a
change on either side shows.

Sizes with max < min or max < avg are refused by cdc_create (the rule has no
defined answer there); none is in the table.
"""
import collections
import math
import os
import re

import numpy as np

import oracle

KIB, MIB = 1 << 10, 1 << 20

# Engine constants restated (fast_engine.cpp, host_common.hpp, small.hpp).
MIN_SPAN_LOG2, MAX_SPAN_LOG2 = 16, 17   # 64 KiB spans, 128 KiB while records stay sparse
SMALL_BATCH = 8 * MIB                   # batches up to this use the small-batch span size
SMALL_MAX_BYTES = 4 * MIB               # the one-launch kernel's longest stream
SMALL_REC_BUDGET = 2048 * 5 // 8        # ... and its expected-record budget (kRecCap * 5 / 8)

SEED = 5

# (min, avg, max, n, twin): n = stream length of the case's inputs; twin = the
# pure-Python oracle twin is fast enough to cross-check the C oracle on a
# <= 200001-byte prefix (min < 100000).  The cases from 100000 up rest on the C
# oracle alone: one chunk of theirs is more than the twin walks in a second.
Case = collections.namedtuple("Case", "min avg max n twin")


def _case(mn, avg, mx, n=None):
    return Case(mn, avg, mx, 3 * mx + mn + 12345 if n is None else n, mn < 100000)


CASES = [
    _case(4097, 8191, 16385),
    _case(65, 257, 1025),
    _case(64, 512, 1024),
    _case(128, 1024, 1048576),
    _case(2000, 3000, 3000),
    _case(3000, 3000, 3000),
    _case(64, 5792, 20001),              # bits 12 ...
    _case(64, 5793, 20001),              # ... and 13: either side of the rounding point 2^12.5
    _case(4096, 32768, 131072),
    _case(32768, 131072, 1048576),
    _case(65536, 262144, 2097152),
    _case(131072, 524288, 4194304),
    _case(262144, 1048576, 8388608),
    _case(524288, 2097152, 16777216),
    _case(1048576, 4194304, 16777216),
    _case(1048576, 1048576, 16777216),
    _case(1048576, 256, 1048576, 8 * 1048576 + 12345),   # every chunk is min = max: 8 of them and a tail
    _case(64, 256, 16777216, 16 * MIB + 70000),           # two spans, both dense: kept to two
    # added for coverage: bits 11, 14 and 16, span_log2 18 and 19, and the
    # parity combinations (odd, even, even), (even, odd, even), (odd, odd,
    # even) and (odd, even, odd)
    _case(1025, 2047, 8192, 6 * 8192 + 1025 + 12345),
    _case(2049, 4096, 16385),
    _case(16385, 65536, 262144, 6 * 262144 + 12345),
    _case(16384, 65537, 524288),
    _case(8192, 16385, 65536),
]

# Not in the table: max / avg = 32 at sparse masks.  A 512 KiB span then expects
# 2^19 / 2^13 = 64 hitting 16-byte pieces, the scan's per-span list length, so
# about every second span of RANDOM data overflows into the exact path and the
# resolve crosses between record lists and overflowed ones all the time.
WIDE_CASE = Case(8192, 16385, 524288, 24 * 524288 + 777, True)

# Further single-stream lengths through the one-launch kernel: a stream shorter
# than max, one shorter than min, and (bits 12, 2^11 expected positions per
# record) one that the (len >> pmin) budget turns away although it is <= 4 MiB.
SMALL_EXTRA = {
    (32768, 131072, 1048576): [MIB + 17, 4 * MIB],
    (1048576, 4194304, 16777216): [MIB + 17, 4 * MIB],
    (2049, 4096, 16385): [3 * MIB + 5],
}

RESOLVE_CASES = [(16384, 65537, 524288), (131072, 524288, 4194304), (524288, 2097152, 16777216),
                 (4097, 8191, 16385)]   # span_log2 19, 22, 24 and the odd triple
WRITE_CASES = [(1048576, 4194304, 16777216), (524288, 2097152, 16777216), (4097, 8191, 16385)]
ASYNC_CASES = [(262144, 1048576, 8388608), (64, 512, 1024)]


def case_of(sizes):
    for c in CASES:
        if (c.min, c.avg, c.max) == tuple(sizes):
            return c
    raise KeyError(sizes)


def sizes_of(case):
    return (case.min, case.avg, case.max)


def case_id(case):
    return f"{case.min}-{case.avg}-{case.max}"


# ---------------------------------------------------------------------------
# The model.

def _masks_table():
    return oracle._tables()[1]


def _popcount(x):
    return bin(x).count("1")


def _ceil_log2(x):
    return (x - 1).bit_length()


def log2_round(avg):
    """lround(log2(avg)): halves away from zero (no integer avg sits on one)."""
    return int(math.floor(math.log2(avg) + 0.5))


Params = collections.namedtuple(
    "Params", "bits mask_s mask_l cmask aligned trunc pop_s pop_l pop_c span_log2 small_span_log2 cap smax "
              "small_on pmin")


def params(mn, avg, mx):
    if mx < mn or mx < avg:
        raise ValueError("FastCDC sizes out of order: max must be >= min and >= avg")
    M = _masks_table()
    bits = log2_round(avg)
    ms, ml = M[bits + 1], M[bits - 1]
    cm = ms & ml
    every = ms | ml
    trunc = every.bit_length() - 1
    assert trunc <= 47
    low = (every & -every).bit_length() - 1
    aligned = low <= 32 and (every >> low) <= 0xFFFFFFFF
    pc = _popcount(cm)
    l2 = _ceil_log2(mx)
    span_log2 = max(l2, MIN_SPAN_LOG2)
    while span_log2 < MAX_SPAN_LOG2 and 11 * ((2 << span_log2) >> pc) <= 384:
        span_log2 += 1
    small_span_log2 = min(max(l2, 14), span_log2)
    span = 1 << span_log2
    cap = min(max(8 * (span >> pc), 64), 256)
    smax = span // ((mn // 2) * 2) + 2
    pmin = min(_popcount(ms), _popcount(ml))
    return Params(bits, ms, ml, cm, aligned, trunc, _popcount(ms), _popcount(ml), pc, span_log2, small_span_log2,
                  cap, smax, pmin >= 10, pmin)


def small_eligible(p, n):
    """FastEngine::small_ok: the one-launch kernel takes a single stream of n bytes."""
    return p.small_on and 0 < n <= SMALL_MAX_BYTES and (n >> p.pmin) <= SMALL_REC_BUDGET


def write_window_bytes():
    """HostPath::kWriteWindow (host_path.hpp): the bytes the streaming write path
    chunks at a time; the last chunk of a window is carried into the next."""
    txt = open(os.path.join(oracle.ROOT, "chunkfs_amd", "csrc", "host_path.hpp")).read()
    m = re.search(r"kWriteWindow = size_t\((\d+)\) << (\d+);", txt)
    return int(m.group(1)) << int(m.group(2))


def batch_span_log2(p, lens):
    """Span size of one batch (FastEngine::enqueue)."""
    return p.small_span_log2 if sum(lens) <= SMALL_BATCH else p.span_log2


def span_count(p, lens):
    """Spans of one batch: per stream, rounded up."""
    sl2 = batch_span_log2(p, lens)
    return sum((n + (1 << sl2) - 1) >> sl2 for n in lens)


SCAN_ENTRIES = 64   # hitting 16-byte pieces the scan lists per span; more overflow the span


def expected_entries(p, lens):
    """16-byte pieces with a (mask_s & mask_l) hit that one span of this batch
    expects on random bytes."""
    return (1 << batch_span_log2(p, lens)) >> p.pop_c


# ---------------------------------------------------------------------------
# Inputs and references, computed once and shared (read-only).

_inputs, _refs = {}, {}


def _frozen(a):
    a.setflags(write=False)
    return a


def zero_region(case):
    """[a, b) of the zero_region input: odd start, one and a half max chunks
    long where the stream has room (random bytes follow it either way)."""
    a = (case.n // 5) | 1
    return a, a + min(case.max + case.max // 2 + 7, (case.n - a) // 2)


def inputs(case):
    """name -> bytes: random; zeros (every cut a max cut: odd max, even re);
    random with a zero region at an unaligned offset, longer than max."""
    key = sizes_of(case)
    if key not in _inputs:
        n = case.n
        rnd = oracle.splitmix64_bytes(n, SEED)
        mixed = rnd.copy()
        a, b = zero_region(case)
        mixed[a:b] = 0
        _inputs[key] = {"random": _frozen(rnd), "zeros": _frozen(np.zeros(n, dtype=np.uint8)),
                        "zero_region": _frozen(mixed)}
    return _inputs[key]


def edge_lengths(case):
    """Single streams at the rule's first thresholds."""
    return [case.min, case.min + 1, (case.min // 2) * 2, case.max + 1]


def data_of(case, name, n=None):
    d = inputs(case)[name]
    return d if n is None else d[:n]


# ---------------------------------------------------------------------------
# Rounding probes.  The rule rounds the remainder and the centre down to even,
# which shows only when a hash hits at exactly the odd position: one time in
# 2^popcount(mask) on random bytes.  These streams put a hit there on purpose.

_M64 = (1 << 64) - 1


def _probe(case, end, want_l, want_s, rng):
    """A first chunk of zero bytes whose last 8 bytes before `end` are chosen
    so that the hash at position end - 1 hits mask_l (want_l) / mask_s (want_s)
    and no earlier position of the tail hits either mask; random bytes follow."""
    g, _ = oracle._tables()
    p = params(*sizes_of(case))
    h0 = 0
    for _ in range(64):                      # the hash inside a long zero run
        h0 = ((h0 << 1) + g[0]) & _M64
    assert h0 & p.mask_l and h0 & p.mask_s   # a zero run never cuts
    while True:
        tail = rng.integers(0, 256, 8, dtype=np.uint8)
        h, ok = h0, True
        for i, b in enumerate(tail.tolist()):
            h = ((h << 1) + g[b]) & _M64
            hit_l, hit_s = h & p.mask_l == 0, h & p.mask_s == 0
            if i < 7:
                ok = ok and not hit_l and not hit_s
            else:
                ok = ok and hit_l == want_l and hit_s == want_s
        if ok:
            break
    head = np.zeros(end, dtype=np.uint8)
    head[end - 8:end] = tail
    return _frozen(np.concatenate([head, oracle.splitmix64_bytes(case.min + 2 * case.avg + 101, SEED + 3)]))


def rounding_probes(case):
    """name -> (data, length of its first chunk under the rule).
    "re": max odd, a mask_l hit at position max - 1, which the rule never
    tests (re = max - 1), so the chunk is max long; a remainder not rounded
    cuts at max - 1.  "ce": avg odd, a hit of mask_l but not of mask_s at
    position avg - 1 = ce, which belongs to the second loop: the chunk is
    avg - 1 long; a centre not rounded tests mask_s there and goes on."""
    key = (sizes_of(case), "probes")
    if key not in _refs:
        rng = np.random.default_rng(case.min * 31 + case.avg * 7 + case.max)
        out = {}
        a0 = (case.min // 2) * 2
        if case.max & 1 and max(a0, case.avg) + 8 < case.max:
            out["re"] = (_probe(case, case.max, True, True, rng), case.max)
        if case.avg & 1 and a0 + 8 < case.avg < case.max:
            out["ce"] = (_probe(case, case.avg, True, False, rng), case.avg - 1)
        _refs[key] = out
    return _refs[key]


def extra(case, n):
    """(data, reference) of a further random stream of n bytes (SMALL_EXTRA)."""
    key = (sizes_of(case), "extra", n)
    if key not in _refs:
        d = _frozen(oracle.splitmix64_bytes(n, SEED + 1))
        _refs[key] = (d, _frozen(oracle.fastcdc(d, *sizes_of(case))))
    return _refs[key]


def ref(case, name, n=None):
    """oracle.fastcdc of inputs(case)[name][:n]."""
    key = (sizes_of(case), name, n)
    if key not in _refs:
        _refs[key] = _frozen(oracle.fastcdc(data_of(case, name, n), *sizes_of(case)))
    return _refs[key]
