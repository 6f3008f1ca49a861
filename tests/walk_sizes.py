"""Size table of the segment-walk chunkers (Rabin / UltraCDC / LeapCDC / SeqCDC
/ AE) and a plain-Python model of what WalkEngine::init derives from a size
triple (a helper of test_walk_sizes_model.py and test_gpu_walk_sizes.py).

The model restates chunkfs_amd/csrc/walk_engine.cpp (init, ensure_workspace,
CallTables::fill) from the code; it imports nothing from it.  The GPU tests
compare cdc_debug_walk_params with it field by field, so a change on either
side shows.

Groups of the table:
  small  4 KiB to 128 KiB segments (seg_log2 12 to 17: a small min lowers it)
         with a large max, so one chunk runs over many segments that hold no
         chunk start.  Each such case names a `pattern` input under which the
         rule cuts (almost) only at max; test_walk_sizes_model.py checks that
         it yields a chunk of 4 segments or more.  Rabin (1, 2, 2), UltraCDC
         (8, 8, 8) and LeapCDC (32, 32, 32) are in this group for the other end
         of it -- min = max at the smallest min a rule takes, the fullest
         per-segment start lists --; no input gives them a chunk longer than
         32 bytes, so they carry no pattern and the long-chunk check is made
         on the second triple of the same rule.
  cap    segments at the 4 MiB cap (seg_log2 22), the warm-up several segments
  top    the top of uint32_t: max = 0xFFFFFFFF, avg next to 2^32
  round  rounding points of rabin_mask / leap_thr, degenerate and odd triples
  fill   further triples so that every seg_log2 from 12 to 22 and both modes of
         Rabin and SeqCDC occur
"""
import collections
import math

import numpy as np

import ae_model
import oracle

KIB, MIB = 1 << 10, 1 << 20
U32 = 0xFFFFFFFF
SEED = 7
ALGOS = ["rabin", "ultra", "leap", "seq", "ae"]
ALGO_ID = {"rabin": 2, "ultra": 4, "leap": 5, "seq": 6, "ae": 7}   # cdc_algo_t

# Engine constants restated (walk.hpp, walk_engine.cpp).
SCAN_BLOCK = 256          # walk::kScanBlock
MAX_FIX_ROUNDS = 16       # walk::kMaxFixRounds
FINISH_MAX = 1 << 16      # segments the fused end kernel takes (walk::finish_fits)
N_MAX = 50 * MIB          # longest input of the table
N_TOP = 6 * MIB           # ... and of the 0xFFFFFFFF cases

# cfg: AE: the window (None = the default for avg); SeqCDC: (mode, seq_length,
# jump_trigger, jump_size) or None for the defaults; else None.
# pattern: None, ("const", byte), ("period", length, seed) or ("counter",).
Case = collections.namedtuple("Case", "algo min avg max n cfg group pattern")


def _case(algo, mn, avg, mx, group, cfg=None, pattern=None, n=None):
    if n is None:
        n = N_TOP if mx == U32 else min(3 * mx + mn + 12345, N_MAX)
    return Case(algo, mn, avg, mx, n, cfg, group, pattern)


CASES = [
    # small segments, long chunks
    _case("seq", 1, 4096, 1048576, "small", pattern=("const", 0)),
    _case("seq", 3, 100, 262144, "small", pattern=("const", 0)),
    _case("rabin", 1, 2, 2, "small"),
    _case("rabin", 16, 4096, 1048576, "small", pattern=("const", 1)),
    _case("ultra", 8, 8, 8, "small"),
    _case("ultra", 8, 4096, 1048576, "small", pattern=("period", 3, 1)),
    _case("leap", 32, 32, 32, "small"),
    _case("leap", 32, 4096, 1048576, "small", pattern=("const", 0x41)),
    _case("ae", 1, 4096, 1048576, "small", pattern=("counter",)),
    # segments at the 4 MiB cap
    _case("seq", 65536, 1048576, 16777216, "cap"),
    _case("ultra", 65536, 1048576, 16777216, "cap"),
    _case("leap", 32768, 262144, 4194304, "cap"),
    _case("ae", 32768, 262144, 4194304, "cap"),
    _case("rabin", 1048576, 4194304, 16777216, "cap"),
    # the top of uint32_t
    _case("rabin", 4096, U32, U32, "top"),
    _case("leap", 32, U32, U32, "top"),
    _case("seq", 4096, 8192, U32, "top"),
    _case("ultra", 4096, 8192, U32, "top"),
    _case("ae", 4096, 8192, U32, "top"),
    # rounding points
    _case("rabin", 64, 5792, 20001, "round"),
    _case("rabin", 64, 5793, 20001, "round"),
    _case("leap", 64, 64 + 5792, 20001, "round"),
    _case("leap", 64, 64 + 5793, 20001, "round"),
    _case("leap", 64, 64, 20001, "round"),          # avg - min = 0
]
for _a in ALGOS:    # degenerate and odd triples, every rule (AE: the default window fits each)
    CASES += [_case(_a, 3000, 3000, 3000, "round"), _case(_a, 2000, 3000, 3000, "round"),
              _case(_a, 4097, 8191, 16385, "round"), _case(_a, 5000, 5001, 5002, "round")]
CASES += [
    _case("seq", 5, 300, 70000, "fill"),                          # seg_log2 14
    _case("ultra", 16, 1000, 50000, "fill"),                      # 16
    _case("ultra", 1000, 20000, 100000, "fill"),                  # 19
    _case("leap", 2000, 40000, 200000, "fill"),                   # 20
    _case("rabin", 10000, 200000, 1000000, "fill"),               # 21
    _case("seq", 300, 1000, 5000, "fill", cfg=(0, 64, 5, 10)),    # seq_length 64: the byte walks
    _case("ae", 100, 400, 1600, "fill", cfg=200),                 # a window that is not the default
]

# One small-segment and one 4 MiB-segment case per rule for the forced schedules.
SCHEDULE_CASES = [c for c in CASES if c.pattern is not None and (c.algo, c.min) != ("seq", 3)] + \
                 [c for c in CASES if c.group == "cap"]
# The write path on the max = 16 MiB cases of two rules (AE's write path is not
# the whole write's chunks, include/chunkfs_amd.h), and the run that follows
# the random half of their second input: a run the rule cuts only at max.
WRITE_CASES = [c for c in CASES if c.group == "cap" and c.algo in ("seq", "rabin")]
WRITE_RUN = {"seq": ("const", 0), "rabin": ("const", 1)}


def sizes_of(case):
    return (case.min, case.avg, case.max)


def case_id(case):
    tail = "" if case.cfg is None else "-" + "_".join(map(str, np.atleast_1d(case.cfg)))
    return f"{case.algo}-{case.min}-{case.avg}-{case.max}{tail}"


def cases(group=None, algo=None):
    return [c for c in CASES if (group is None or c.group == group) and (algo is None or c.algo == algo)]


# ---------------------------------------------------------------------------
# The model.

def _ceil_log2(x):
    return (x - 1).bit_length()


def log2_round(x):
    """round(log2 x) of an integer x >= 1 (no integer sits on a half), from the
    floating-point logarithm checked against exact integer squares."""
    b = int(math.floor(math.log2(x) + 0.5))
    assert (x * x >= 1 << (2 * b - 1) if b else x == 1) and x * x < 1 << (2 * b + 1), x
    return b


Params = collections.namedtuple(
    "Params", "nbm mode warm_mult seg_log2 warm cap piece_log2 seg_words rabin_mask leap_index leap_thr window")


def params(algo, mn, avg, mx, cfg=None, walk_bytes=False, walk=None):
    """What WalkEngine::init derives.  walk_bytes: CHUNKFS_AMD_WALK_BYTES=1;
    walk: CHUNKFS_AMD_WALK as (seg_log2, warm_over_avg).  ValueError where
    validate() refuses."""
    P = oracle._cdc_params()
    if not (0 < mn <= avg <= mx) or (algo == "ultra" and mn < 8) or (algo == "leap" and mn < 32) or \
            (algo == "rabin" and avg < 2):
        raise ValueError("invalid sizes")
    window = 0
    if algo == "ae":
        window = ae_model.default_window(avg) if cfg is None else cfg
        if window < 1 or window + 1 > mx:
            raise ValueError("invalid AE config")
    seq_length = cfg[1] if algo == "seq" and cfg is not None else P["CDC_SEQ_LENGTH"]
    if algo == "rabin":
        nbm = 1 if mn >= P["CDC_RABIN_WINDOW"] else 0
    elif algo == "seq":
        nbm = 1 if seq_length <= 63 else 0
    else:
        nbm = {"ultra": 3, "leap": 2, "ae": 1}[algo]
    if walk_bytes and algo != "ae":
        nbm = 0
    if not nbm:
        warm_mult = 16 if algo == "seq" else 8
        seg_log2 = 15
    else:
        warm_mult = 8 if algo == "rabin" else 24 if algo == "leap" else 16
        seg_log2 = 17 if algo == "rabin" else 18
        wl = _ceil_log2(warm_mult * avg)
        if wl > seg_log2:                       # at least the warm-up, up to 4 MiB
            seg_log2 = min(wl, 22)
    lmin = mn.bit_length() - 1 + 12             # start list: segment / min + 2 <= ~4k entries
    if seg_log2 > lmin:
        seg_log2 = max(lmin, 12)
    if walk is not None and 10 <= walk[0] <= 30:
        seg_log2, warm_mult = walk
    if algo == "ae" and seg_log2 < 12:
        seg_log2 = 12
    seg = 1 << seg_log2
    li = min(log2_round(avg - mn if avg > mn else 1), 32)
    return Params(nbm, "bitmap" if nbm else "byte", warm_mult, seg_log2, warm_mult * avg, (seg // mn + 2) & U32,
                  min(seg_log2, 15), seg // 64, (1 << log2_round(avg)) - 1, li, P["THR"][li], window)


def debug_words(p):
    """The first seven values of cdc_debug_walk_params."""
    return [p.nbm, p.seg_log2, p.warm, p.cap, p.piece_log2, p.rabin_mask, p.leap_thr]


def segments(p, lens):
    """Segments of one batch: per stream, rounded up (CallTables::fill)."""
    return sum((n + (1 << p.seg_log2) - 1) >> p.seg_log2 for n in lens)


def workspace_per_segment(algo, p, quiet=True, bits_fine=True):
    """Bytes of WalkEngine::ensure_workspace that grow with the segment count."""
    P = oracle._cdc_params()
    b = 5 * 8 + 4 + p.cap * 8 + 8 / SCAN_BLOCK           # E X Xs Es P, N, the start list, block sums
    b += p.seg_words * p.nbm * 8                         # predicate bitmaps
    if algo == "leap" and p.nbm:
        b += p.seg_words * 30                            # word tables and 512-position block tables
    rsum = bool(p.nbm) and 12 <= p.piece_log2 <= 15 and quiet
    if algo == "rabin":
        rsum = rsum and p.rabin_mask <= U32 and P["CDC_RABIN_POLY"].bit_length() - 1 - 8 >= 32
    elif algo == "ae":
        rsum = False
    else:
        rsum = rsum and bits_fine
    if rsum:
        b += p.seg_words // 8 * (2 if algo == "rabin" else 1) + 1
    if algo == "ae":
        b += p.seg_words * 4 + p.seg_words // 64 * 4
    return b


def workspace_bytes(algo, p, segs, streams, **kw):
    """The arena of a first batch of `segs` segments and `streams` streams
    (its 256-byte alignment gaps left out: under 5 KiB)."""
    S, N = segs + segs // 4 + 16, streams + 64
    return int(S * workspace_per_segment(algo, p, **kw)) + (N + 1) * 8 * 4 + (4 + 4 * MAX_FIX_ROUNDS) * 8 + 16


# ---------------------------------------------------------------------------
# Inputs and references, computed once and shared (read-only).

_inputs, _refs = {}, {}


def _frozen(a):
    a.setflags(write=False)
    return a


def make_pattern(spec, n):
    if spec[0] == "const":
        return np.full(n, spec[1], dtype=np.uint8)
    if spec[0] == "period":
        return np.resize(oracle.splitmix64_bytes(spec[1], spec[2]), n)
    if spec[0] == "counter":                 # big-endian 32-bit counter: 0, 1, 2, ...
        return np.arange((n + 3) // 4, dtype=">u4").view(np.uint8)[:n].copy()
    raise ValueError(spec)


def zero_region(case):
    """[a, b) of the zero_region input: odd start, one and a half max chunks
    long where the stream has room (random bytes follow it either way)."""
    a = (case.n // 5) | 1
    return a, a + min(case.max + case.max // 2 + 7, (case.n - a) // 2)


def inputs(case):
    """name -> bytes: random; zeros; random with a zero region at an unaligned
    offset; the case's pattern where it has one."""
    key = case
    if key not in _inputs:
        n = case.n
        rnd = oracle.splitmix64_bytes(n, SEED)
        mixed = rnd.copy()
        a, b = zero_region(case)
        mixed[a:b] = 0
        d = {"random": _frozen(rnd), "zeros": _frozen(np.zeros(n, dtype=np.uint8)), "zero_region": _frozen(mixed)}
        if case.pattern is not None:
            d["pattern"] = _frozen(make_pattern(case.pattern, n))
        _inputs[key] = d
    return _inputs[key]


def input_names(case):
    return ["random", "zeros", "zero_region"] + (["pattern"] if case.pattern is not None else [])


def reference(case, data):
    """The rule's chunks of one buffer: oracle.cdc, or the AE model."""
    if case.algo == "ae":
        return ae_model.chunk_array(data, case.min, case.avg, case.max, case.cfg)
    return oracle.cdc(case.algo, data, case.min, case.avg, case.max, seqcfg=case.cfg)


def ref(case, name):
    key = (case, name)
    if key not in _refs:
        _refs[key] = _frozen(reference(case, inputs(case)[name]))
    return _refs[key]


def write_inputs(case):
    """name -> (bytes, chunks of the whole write): random; its first half (odd
    length), then the case's WRITE_RUN to the end."""
    key = (case, "write")
    if key not in _refs:
        rnd = inputs(case)["random"]
        half = (case.n // 2) | 1
        tail = np.concatenate([rnd[:half], make_pattern(WRITE_RUN[case.algo], case.n - half)])
        _refs[key] = {"random": (rnd, ref(case, "random")), "random_then_run": (_frozen(tail), reference(case, tail))}
    return _refs[key]


# ---------------------------------------------------------------------------
# The batch of more than 2^16 segments (test_gpu_walk_sizes.py).  4 KiB
# segments (CHUNKFS_AMD_WALK="12,2"): one per stream of 1 to 4096 bytes.
#
# The batch is to end in the gated output behind the first fix-up round, which
# runs only when that round changes no segment's exit: every re-walked chain
# has to meet the chain it replaces before its segment ends.  And the round is
# to have segments to walk again: guessed chains that have not met the true one
# when their segment begins.  So the long streams hold bytes under which the
# rule cuts on content every few dozen bytes: random bytes for Rabin, LeapCDC
# and AE; for UltraCDC bytes one bit off its pattern 0xAA now and then (on
# random bytes it cuts at max only: the distance to the pattern is almost never
# 0 under its masks); for SeqCDC runs that climb by one (on random bytes five
# increasing bytes are rare and its jumps skip most of them).  And max is a
# fraction of the segment and no divisor of it: a walk starts on the stream's
# max-length grid, `warm` bytes or more before its segment, so max = 4096
# would give every walk a whole segment of warm-up and nothing to fix.
# rounds_settle_at_once() predicts the first round on the CPU;
# test_walk_sizes_model.py holds it at "some segments walked again, no exit
# changed" for every rule.

BIG_WALK = (12, 2)
BIG_STREAMS = 66000
BIG_LONG = 300
BIG = {   # rule -> (sizes, kind of the long streams' bytes)
    "rabin": ((64, 256, 1000), "random"),
    "ultra": ((16, 64, 520), "near_aa"),
    "leap": ((32, 96, 1000), "random"),
    "seq": ((16, 64, 520), "climb"),
    "ae": ((64, 256, 300), "random"),
}


def big_case(algo, sizes=None):
    return Case(algo, *(sizes or BIG[algo][0]), 0, None, "big", None)


def big_long_bytes(kind, n, seed):
    rnd = oracle.splitmix64_bytes(2 * n, seed)
    if kind == "random":
        return rnd[:n]
    if kind == "near_aa":       # 0xAA, one bit flipped in every fourth byte or so
        flip = np.where(rnd[:n] < 64, np.uint8(1) << (rnd[n:] & 7), 0).astype(np.uint8)
        return np.uint8(0xAA) ^ flip
    if kind == "climb":         # b[i+1] = b[i] + 1 four times in five, else a random byte
        idx = np.arange(n)
        reset = rnd[n:] >= 205
        reset[0] = True
        last = np.maximum.accumulate(np.where(reset, idx, 0))     # where the current climb began
        return ((rnd[:n][last].astype(np.int64) + idx - last) & 0xFF).astype(np.uint8)
    raise ValueError(kind)


_big = {}


def big_batch(kind):
    """(lens, the bytes of every stream) of the batch whose long streams hold
    `kind` bytes; the short ones are random."""
    if kind not in _big:
        lens = big_batch_lengths()
        offs = np.concatenate([[0], np.cumsum(lens)])
        host = oracle.splitmix64_bytes(int(offs[-1]) + 16, 2025)
        _big[kind] = (lens, [_frozen(big_long_bytes(kind, n, 3000 + i)) if n >= 20000 else host[offs[i]:offs[i] + n]
                             for i, n in enumerate(lens)])
    return _big[kind]


def rounds_settle_at_once(case, data, seg_log2, warm):
    """(walked again, exits changed): how many segments of one stream the first
    fix-up round walks again, and how many of them it leaves with a changed
    exit.  Segment k is first walked from start(k), `warm` bytes or more before
    it, as if a chunk began there; its entry is that chain's first chunk start
    in k or later, its exit the first one past k.  Its predecessor's exit comes
    from the chain that began at start(k - 1).  Where entry and the
    predecessor's exit differ, the round walks k again along the predecessor's
    chain; the exit changes unless the two chains have met by the end of k."""
    seg, n, again, changed = 1 << seg_log2, len(data), 0, 0

    def chain(a, e):
        b = min(n, e + 3 * case.max)                # (cuts up to e + max read no byte past that)
        r = reference(case, data[a:b])
        return np.concatenate([r[:, 0] + np.uint64(a), [b]]).astype(np.uint64)

    def first_from(c, x):
        return int(c[c >= x][0])

    def start(s):                                   # walk.hip: `warm` bytes back, on the stream's max-length grid
        return max(0, s - warm) // case.max * case.max

    for s in range(seg, n, seg):
        e = min(n, s + seg)
        own, pred = chain(start(s), e), chain(start(s - seg), e)
        if first_from(own, s) != first_from(pred, s):
            again += 1
            changed += first_from(own, e) != first_from(pred, e)
    return again, changed


def big_batch_lengths():
    """About 66000 stream lengths: most 0 to 200 bytes, every 97th empty, 300 of
    20 KB to 200 KB, the last five empty.  A long stream ends up to 60 bytes
    short of a 4 KiB segment border: a last segment of a few bytes would leave
    a re-walked chain only the warm-up (2 avg) to meet the one it replaces,
    and the first round would not settle (see BIG below)."""
    rng = np.random.default_rng(2024)
    lens = rng.integers(0, 201, BIG_STREAMS)
    lens[::97] = 0
    where = rng.choice(np.arange(1, BIG_STREAMS - 5), BIG_LONG, replace=False)
    where = where[where % 97 != 0]
    lens[where] = rng.integers(5, 49, len(where)) * 4096 - where % 61
    lens[-5:] = 0
    return [int(x) for x in lens]


def trim_to_segments(lens, seg_log2, want):
    """A prefix of lens, its last stream shortened, with exactly `want`
    segments (streams dropped from the end)."""
    out, segs = [], 0
    for n in lens:
        k = (n + (1 << seg_log2) - 1) >> seg_log2
        if segs + k > want:
            out.append((want - segs) << seg_log2)
            segs = want
            break
        out.append(n)
        segs += k
    assert segs == want, "the batch is shorter than that"
    return out
