"""CPU guard of the FastCDC size table (tests/fast_sizes.py): the table covers
the engine's whole parameter range, the oracle and its Python twin agree on
it, and every case's input makes the chunk list depend on the masks.

What the GPU suite then runs over the table is test_gpu_fast_sizes.py."""
import itertools

import pytest

import fast_sizes as fs
import oracle

ALL = [(c, fs.params(*fs.sizes_of(c))) for c in fs.CASES]


def test_table_is_valid_and_unique():
    seen = set()
    for c, _ in ALL:
        assert 64 <= c.min <= 1048576 and 256 <= c.avg <= 4194304 and 1024 <= c.max <= 16777216, c
        assert c.max >= c.min and c.max >= c.avg, c   # cdc_create refuses the rest
        assert fs.sizes_of(c) not in seen
        seen.add(fs.sizes_of(c))
        assert c.twin == (c.min < 100000)
    for group in (fs.RESOLVE_CASES, fs.WRITE_CASES, fs.ASYNC_CASES, fs.SMALL_EXTRA):
        for sizes in group:
            fs.case_of(sizes)


def test_model_refuses_undefined_orderings():
    for sizes in [(1048576, 256, 1024), (2048, 1024, 1024), (64, 4194304, 1024)]:
        with pytest.raises(ValueError):
            fs.params(*sizes)


def test_model_known_rows():
    """Rows worked out by hand from fast_engine.cpp and the mask table."""
    p = fs.params(4096, 8192, 16384)
    assert (p.bits, p.aligned, p.trunc, p.pop_c, p.span_log2, p.small_span_log2, p.cap, p.smax, p.small_on) == \
        (13, True, 47, 12, 17, 14, 256, 34, True)
    p = fs.params(64, 256, 1024)
    assert (p.bits, p.aligned, p.trunc, p.pop_c, p.span_log2, p.cap, p.smax, p.small_on) == \
        (8, False, 40, 2, 16, 256, 1026, False)
    p = fs.params(16384, 65536, 65536)
    assert (p.bits, p.aligned, p.pop_c, p.span_log2, p.cap) == (16, False, 14, 17, 64)
    p = fs.params(64, 256, 16777216)
    assert (p.span_log2, p.small_span_log2, p.smax) == (24, 24, 262146)
    assert fs.write_window_bytes() == 256 << 20


def test_coverage_of_the_parameter_range():
    P = [p for _, p in ALL]
    assert {p.bits for p in P} == set(range(8, 23))
    assert {p.span_log2 for p in P} == set(range(16, 25))
    assert {p.cap for p in P if p.span_log2 == 24} == {64, 128, 256}
    assert {p.aligned for p in P} == {True, False}
    assert {p.trunc for p in P} == {40, 46, 47}
    assert {p.small_on for p in P} == {True, False}
    # the general form at trunc 47 both below and above the aligned range
    assert any(not p.aligned and p.bits < 11 and p.trunc == 47 for p in P)
    assert any(not p.aligned and p.bits > 14 for p in P)
    # min, the centre (avg) and the remainder (max on a max cut) are each
    # rounded down to even: every parity combination of the three
    assert {(c.min & 1, c.avg & 1, c.max & 1) for c, _ in ALL} == set(itertools.product((0, 1), repeat=3))
    # record density: the avg <= 1024 masks overflow every span of random
    # bytes (the scan lists 64 hitting pieces per span), the others expect at
    # most 32, so an overflow there is a > 5 sigma event
    for c, p in ALL:
        e = fs.expected_entries(p, [c.n])
        assert e >= 4 * fs.SCAN_ENTRIES if c.avg <= 1024 else e <= fs.SCAN_ENTRIES // 2, c
    w = fs.WIDE_CASE
    assert fs.expected_entries(fs.params(*fs.sizes_of(w)), [w.n]) == fs.SCAN_ENTRIES
    # min > avg (an empty first loop), min == max and avg == max stay valid
    assert any(c.min > c.avg for c, _ in ALL)
    assert any(c.min == c.max for c, _ in ALL) and any(c.avg == c.max for c, _ in ALL)


def _small_lengths(c):
    return [c.n] + fs.edge_lengths(c) + fs.SMALL_EXTRA.get(fs.sizes_of(c), [])


def test_coverage_of_the_small_kernel():
    """Off (sparse-hit budgets do not hold), on and taken, and on but turned
    away by the (len >> pmin) record budget at a length the kernel could hold."""
    taken = [(c, n) for c, p in ALL for n in _small_lengths(c) if fs.small_eligible(p, n)]
    off = [(c, n) for c, p in ALL for n in _small_lengths(c) if not p.small_on]
    budget = [(c, n) for c, p in ALL for n in _small_lengths(c)
              if p.small_on and n <= fs.SMALL_MAX_BYTES and not fs.small_eligible(p, n)]
    too_long = [(c, n) for c, p in ALL for n in _small_lengths(c) if p.small_on and n > fs.SMALL_MAX_BYTES]
    assert taken and off and budget and too_long
    # through the kernel: a stream shorter than max and one shorter than min
    assert any(n < c.max and n > c.min for c, n in taken)
    assert any(n < c.min for c, n in taken)
    assert any(n == fs.SMALL_MAX_BYTES for c, n in taken)


def test_rounding_boundary_of_log2_avg():
    a, b = fs.case_of((64, 5792, 20001)), fs.case_of((64, 5793, 20001))
    assert fs.params(*fs.sizes_of(a)).bits == 12 and fs.params(*fs.sizes_of(b)).bits == 13
    assert a.n == b.n == 72412 and fs.SEED == 5
    ra, rb = fs.ref(a, "random"), fs.ref(b, "random")
    assert (len(ra), len(rb)) == (20, 14)
    assert ra.tolist() != rb.tolist()


@pytest.mark.parametrize("case", [c for c in fs.CASES + [fs.WIDE_CASE] if c.twin], ids=fs.case_id)
def test_oracle_twin_agrees(case):
    sizes = fs.sizes_of(case)
    for name in ("random", "zero_region"):
        data = fs.data_of(case, name)[:200001]
        ref = fs.ref(case, name) if len(data) == case.n else oracle.fastcdc(data, *sizes)
        assert oracle.py_fastcdc(data, *sizes).tolist() == ref.tolist(), (sizes, name)
    for n in fs.edge_lengths(case):
        if n <= 200001:
            data = fs.data_of(case, "random", n)
            assert oracle.py_fastcdc(data, *sizes).tolist() == oracle.fastcdc(data, *sizes).tolist(), (sizes, n)


@pytest.mark.parametrize("case", fs.CASES + [fs.WIDE_CASE], ids=fs.case_id)
def test_enough_chunks_and_a_mask_cut(case):
    """>= 8 chunks of random data, which tile it; one of them, not the tail,
    ends at a mask hit: longer than the even-rounded min (the first tested
    position) and shorter than max.  With (min/2)*2 >= (max/2)*2 the rule tests
    no position at all -- every chunk is max -- and the case is there for
    exactly that."""
    r = fs.ref(case, "random")
    assert len(r) >= 8
    assert int(r[0, 0]) == 0 and int(r[:, 1].sum()) == case.n
    assert (r[1:, 0] == r[:-1, 0] + r[:-1, 1]).all()
    a0 = (case.min // 2) * 2
    mask_cuts = [int(x) for x in r[:-1, 1] if a0 < int(x) < case.max]
    if a0 >= (case.max // 2) * 2:
        assert not mask_cuts and set(r[:-1, 1].tolist()) == {case.max}
    else:
        assert mask_cuts
    # zeros: the placeholder GEAR never hits on a constant run, so every cut
    # is a max cut (an odd max stays odd: the remainder is not rounded)
    z = fs.ref(case, "zeros")
    assert set(z[:-1, 1].tolist()) == {case.max}
    zr = fs.ref(case, "zero_region")
    a, b = fs.zero_region(case)
    assert a & 1 and 0 < a < b < case.n
    # the chunk that runs into the region ends at max or at the region's end
    # (a cut in the first 63 zero bytes still sees the bytes before them)
    assert int(zr[:, 1].max()) >= min(case.max, b - a - 64)


def _variant(data, mn, avg, mx, small_shift=1, round_a0=True, round_ce=True, round_re=True):
    """The rule with one thing changed: MASKS[bits + small_shift] for the
    first loop, or min / centre / remainder not rounded down to even."""
    g, M = oracle._tables()
    bits = fs.log2_round(avg)
    ms, ml = M[bits + small_shift], M[bits - 1]
    d, out, pos = bytes(bytearray(data)), [], 0
    while pos < len(d):
        rem = len(d) - pos
        cut = rem
        if rem > mn:
            center = avg
            if rem > mx:
                rem = mx
            elif rem < center:
                center = rem
            a0 = (mn // 2) * 2 if round_a0 else mn
            ce = (center // 2) * 2 if round_ce else center
            re_ = (rem // 2) * 2 if round_re else rem
            h, cut = 0, rem
            for p in range(a0, re_):
                h = ((h << 1) + g[d[pos + p]]) & ((1 << 64) - 1)
                if h & (ms if p < ce else ml) == 0:
                    cut = p
                    break
        out.append([pos, cut])
        pos += cut
    return out


def test_wrong_mask_or_min_rounding_changes_the_table_data():
    """The guard has teeth: MASKS[bits] in place of MASKS[bits + 1], or an odd
    min not rounded down, gives another chunk list on the table's random data."""
    c = fs.case_of((64, 5793, 20001))
    good = fs.ref(c, "random").tolist()
    assert _variant(fs.data_of(c, "random"), *fs.sizes_of(c)) == good
    assert _variant(fs.data_of(c, "random"), *fs.sizes_of(c), small_shift=0) != good
    c = fs.case_of((65, 257, 1025))
    good = fs.ref(c, "random").tolist()
    assert _variant(fs.data_of(c, "random"), *fs.sizes_of(c)) == good
    assert _variant(fs.data_of(c, "random"), *fs.sizes_of(c), round_a0=False) != good


def test_rounding_probes_discriminate():
    """Every odd max and every odd avg of the table has a stream on which the
    rule and the rule without that rounding differ in the first chunk."""
    seen = {"re": 0, "ce": 0}
    for c in fs.CASES:
        probes = fs.rounding_probes(c)
        if c.twin:
            assert ("re" in probes) == bool(c.max & 1 and max((c.min // 2) * 2, c.avg) + 8 < c.max), c
            assert ("ce" in probes) == bool(c.avg & 1 and (c.min // 2) * 2 + 8 < c.avg < c.max), c
        for kind, (data, first_len) in probes.items():
            sizes = fs.sizes_of(c)
            ref = oracle.fastcdc(data, *sizes)
            assert int(ref[0, 1]) == first_len, (c, kind)
            if not c.twin:
                continue
            seen[kind] += 1
            assert oracle.py_fastcdc(data, *sizes).tolist() == ref.tolist()
            bad = _variant(data, *sizes, round_re=False) if kind == "re" else _variant(data, *sizes, round_ce=False)
            assert bad[0][1] != first_len and bad != ref.tolist(), (c, kind)
            assert bad[0][1] == c.max - 1 if kind == "re" else bad[0][1] > c.avg - 1
    assert seen["re"] >= 4 and seen["ce"] >= 4
