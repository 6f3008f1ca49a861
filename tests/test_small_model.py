"""The numpy model of the one-launch FastCDC kernel (tests/small_model.py)
against the sequential oracle, on the CPU, and the coverage conditions of
tests/test_gpu_small_stages.py: every input the GPU file uses is chunked here
by the model's chain and compared with oracle.fastcdc, and every path an input
was chosen for (a region known in its own block, in the next one, only in the
last; heads; max-cut runs over more than one link round; trunc_load's guarded
branch; the record budgets at and one past their edge) is asserted from the
model, so a GPU test cannot quietly stop reaching it."""
import collections

import numpy as np
import pytest

import fast_sizes as fs
import oracle
import small_model as sm


def _same(model, ref, what):
    got = model.chunks()
    assert got.shape == ref.shape and (got == ref).all(), what


def test_geometry_constants_read_from_the_kernel():
    assert sm.BLOCK_BYTES == 8 * sm.PIECE and sm.BLOCK_BYTES * sm.MAX_BLOCKS == fs.SMALL_MAX_BYTES
    assert sm.REC_CAP * 5 // 8 == fs.SMALL_REC_BUDGET
    assert sm.ENT_CAP > sm.REC_CAP >= sm.BLOCK_REC_CAP > sm.LANE_HITS > 0 and sm.ROUNDS > 2


@pytest.mark.parametrize("sizes", sm.SCAN_SETS, ids=sm.set_id)
def test_scan_inputs_chain_and_paths(sizes):
    """(a), (g): the chain equals the oracle; the inputs hold regions of every
    class the set can have, heads and a max-cut run."""
    p = fs.params(*sizes)
    where, heads, run = collections.Counter(), 0, 0
    for name in sm.SCAN_DATA + ["random2"]:
        scan = sm.scan_of(sizes, name)
        n = scan.buf.size
        assert fs.small_eligible(p, n) and 2 <= -(-n // sm.BLOCK_BYTES)
        m = scan.model()
        _same(m, sm.ref_of(scan, n, (sizes, name)), (sizes, name))
        ch = m.chain()
        heads, run = heads + len(ch.heads), max(run, ch.max_run)
        if not m.fallback():
            where.update(m.where_counts())
        # the short call of the scratch-history test
        _same(scan.model(40 * sm.KIB), sm.ref_of(scan, 40 * sm.KIB, (sizes, name)), (sizes, name, "40 KiB"))
    assert not sm.scan_of(sizes, "random").model().fallback()
    assert where[sm.NEXT] > 0 and heads > 0 and run >= 1
    if sizes[0] < sm.BLOCK_BYTES:
        assert where[sm.OWN] > 0      # (min >= a block: every region lies past its record's block)
    print(sizes, dict(where), "heads", heads, "longest run", run)


@pytest.mark.parametrize("sizes", sm.SCAN_SETS, ids=sm.set_id)
def test_sweeps_chain_and_paths(sizes):
    """(b), (d): one byte at a time across the tail-chunk rule, a block edge
    and a piece edge; the end sweep has streams on both sides of n - c = min
    and streams whose last live chunk is in the end regime (rem < avg)."""
    scan, c = sm.scan_of(sizes, "random"), sm.sweep_start(sizes)
    assert c // sm.BLOCK_BYTES >= 2
    sweeps = sm.sweep_lengths(sizes)
    assert [len(v) for v in sweeps.values()] == [133, 141, 141]
    assert set(sm.align_lengths(sizes)) <= set(sweeps["end"]) and len(sm.align_lengths(sizes)) == 10
    tail = live = end_regime = mem = 0
    for kind, lens in sweeps.items():
        for n in lens:
            m = scan.model(n)
            _same(m, sm.ref_of(scan, n, (sizes, "random")), (sizes, kind, n))
            if kind == "end":
                ch = m.chain()
                if c in ch.starts:
                    tail += not m.live(c)
                    live += m.live(c)
                    end_regime += m.live(c) and n - c < sizes[1]
                mem += len(ch.mem_starts) > 0
    assert tail >= 2 and live >= 100 and end_regime >= 100
    print(sizes, "end sweep: tail", tail, "live", live, "end regime", end_regime, "memory loads in", mem, "calls")


def _guard_counts(scan, lens):
    inside = outside = 0
    for n in lens:
        m = scan.model(n)
        g = m.guarded_starts(n)
        inside += len(g) > 0
        outside += len(g) == 0 and len(m.chain().mem_starts) > 0
    return inside, outside


@pytest.mark.parametrize("sizes,k", sm.GUARD_ZERO, ids=lambda v: sm.set_id(v) if isinstance(v, tuple) else str(v))
def test_guarded_load_zero_streams(sizes, k):
    """(c): zero bytes, the default GEAR table: every cut is a max cut, every
    start but offset 0 a head whose region the last block loads from memory."""
    lens = sm.guard_zero_lengths(sizes, k)
    scan = sm.zeros_scan(sizes, max(lens))
    assert k * sizes[2] > 2 * sm.BLOCK_BYTES        # the run spans blocks
    for n in lens:
        m = scan.model(n)
        _same(m, sm.ref_of(scan, n, (sizes, "zeros")), (sizes, n))
        ch = m.chain()
        assert m.rec.size == 1 and len(ch.heads) == len(ch.starts) - 1 >= k - 1
        assert not m.fallback()
    inside, outside = _guard_counts(scan, lens)
    assert inside >= 16 and outside >= 16, (inside, outside)
    print(sizes, "guarded calls", inside, "unguarded", outside)


def test_guarded_load_record_two_blocks_before_its_region():
    """(c): random bytes, min = 32 KiB: the record s ends a block, so its
    region is out of the next block's reach and the last block loads it."""
    scan, s, lens = sm.guard_random()
    assert fs.small_eligible(scan.p, max(lens))
    for n in lens:
        m = scan.model(n)
        _same(m, sm.ref_of(scan, n, (scan.sizes, "guard_random")), n)
        if m.live(s) and m.regime(s).tl > m.regime(s).a0:
            assert s in m.chain().starts and m.trunc_of(s).own_where == sm.LAST
            assert s in m.chain().mem_starts
    inside, outside = _guard_counts(scan, lens)
    assert inside >= 16 and outside >= 16, (inside, outside)
    print("guarded calls", inside, "unguarded", outside)


def test_budget_edges():
    """(e): exactly at and one past the three record budgets."""
    cases = sm.budget_cases()
    want = {f"lane_{sm.LANE_HITS}": None, f"lane_{sm.LANE_HITS + 1}": "lane",
            f"block_{sm.BLOCK_REC_CAP}": None, f"block_{sm.BLOCK_REC_CAP + 1}": "block",
            f"call_{sm.REC_CAP}": None, f"call_{sm.REC_CAP + 1}": "call"}
    assert set(cases) == set(want) | {"entries_over"}
    for name, scan in cases.items():
        if name not in want:
            continue
        m = scan.model()
        assert fs.small_eligible(scan.p, scan.buf.size)
        assert m.record_fallback() == want[name], name
        assert not m.chain_fallback()
        _same(m, sm.ref_of(scan, scan.buf.size, (name, "gear0")), name)
    m = cases[f"lane_{sm.LANE_HITS}"].model()
    assert m.lane_counts().max() == sm.LANE_HITS
    assert cases[f"lane_{sm.LANE_HITS + 1}"].model().lane_counts().max() == sm.LANE_HITS + 1
    for t in (sm.BLOCK_REC_CAP, sm.BLOCK_REC_CAP + 1):
        m = cases[f"block_{t}"].model()
        per = sm.BLOCK_BYTES // sm.LANE_BYTES
        assert m.lane_counts().max() <= sm.LANE_HITS and int(m.lane_counts()[per:2 * per].sum()) == t
        assert m.rec.size <= sm.REC_CAP
    for t in (sm.REC_CAP, sm.REC_CAP + 1):
        m = cases[f"call_{t}"].model()
        assert m.rec.size == t and m.lane_counts().max() <= sm.LANE_HITS
        assert m.block_counts().max() <= sm.BLOCK_REC_CAP


def test_entry_budget_and_link_rounds():
    """(f): zero streams whose heads fill at most half of the entries kept for
    starts that are not records, in runs longer than one round adds."""
    for sizes, n in sm.ENTRY_CASES[:2]:
        assert fs.small_eligible(fs.params(*sizes), n)
        scan = sm.zeros_scan(sizes, n)
        m = scan.model()
        ch = m.chain()
        _same(m, sm.ref_of(scan, n, (sizes, "zeros")), (sizes, n))
        entries, rounds, failed = m.link_stage()
        assert len(ch.heads) <= sm.HEAD_BUDGET // 2 and ch.max_run > sm.RUN_LEN and rounds > 1
        assert entries == 1 + len(ch.heads) and not failed and not m.fallback()
        print(sizes, n, "heads", len(ch.heads), "rounds", rounds)


def test_entry_budget_is_out_of_an_eligible_zero_streams_reach():
    """The other half of (f) -- heads at least double that budget -- cannot be
    built: a handle takes the small kernel only when min(popcount) >= 10, a
    stream only when n >> pmin <= kRecCap * 5 / 8, and max >= avg ~ 2^(pmin+1):
    a zero stream has at most n / max < 5 / 8 * kRecCap / 2 + 1 heads.  The
    third entry case is that bound: still within the entry and round budgets,
    so the model predicts no fallback."""
    sizes, n = sm.ENTRY_CASES[2]
    p = fs.params(*sizes)
    assert p.small_on and p.pmin == 10 and sizes[2] == sizes[1]
    assert fs.small_eligible(p, n) and not fs.small_eligible(p, n + sizes[2])
    scan = sm.zeros_scan(sizes, n)
    m = scan.model()
    ch = m.chain()
    _same(m, sm.ref_of(scan, n, (sizes, "zeros")), (sizes, n))
    entries, rounds, failed = m.link_stage()
    assert sm.HEAD_BUDGET // 2 < len(ch.heads) < 2 * sm.HEAD_BUDGET
    assert entries <= sm.ENT_CAP and rounds <= sm.ROUNDS // 2 and not failed and not m.fallback()


def test_entry_budget_exceeded_by_truncated_hits():
    """What a zero stream cannot do, dense records can: with zero bytes min
    after them their links are truncated hits, each a head entry, and the
    records and heads together are past the entry budget while every record
    budget holds."""
    scan = sm.budget_cases()["entries_over"]
    m = scan.model()
    assert fs.small_eligible(scan.p, scan.buf.size)
    entries, rounds, failed = m.link_stage()
    assert m.record_fallback() is None and failed and m.fallback()
    assert m.rec.size <= sm.REC_CAP and entries > sm.ENT_CAP, entries
    _same(m, sm.ref_of(scan, scan.buf.size, ("entries_over", "gear0")), "entries_over")


def test_end_region_in_front_of_a_piece_the_stream_never_reaches():
    """The region of the record at c ends with the stream just below a 4 KiB
    piece edge, and its 52 word-aligned bytes reach into the piece past that
    edge, which has no byte of the stream: a block evaluating the region reads
    the 64 bytes in front of a piece it never loads."""
    classes = collections.Counter()
    for name, scan, n, c in sm.piece_end_cases():
        m = scan.model(n)
        _same(m, sm.ref_of(scan, n, (name, "gear0")), name)
        assert not m.fallback() and c in m._index
        t = m.trunc_of(c)
        assert t.own == 0                       # zero bytes, GEAR[0] = 0: a hit at the region's first position
        a = (c + m.regime(c).a0) & ~3
        edge = -(-n // sm.PIECE) * sm.PIECE
        assert n <= edge <= a + sm.REGION_SPAN - 1
        classes[t.own_where] += 1
    assert classes[sm.OWN] >= 2 and classes[sm.NEXT] >= 1 and classes[sm.LAST] >= 1, classes


# ---- the comparisons discriminate ---------------------------------------------

def _readout(sizes, name, n=None):
    m = sm.Scan(sm.scan_input(sizes, name), sizes).model(n)
    return [m.block_regions(b).tolist() for b in range(m.blocks)]


def test_one_constant_off_changes_what_the_gpu_tests_compare(monkeypatch):
    """A model with one constant changed gives another read-out, another
    guarded-branch set or another fallback prediction on the GPU tests' own
    inputs: were the kernel off by that much, the comparison would fail."""
    sizes = sm.SCAN_SETS[0]
    true_regions = _readout(sizes, "random")
    scan, s, lens = sm.guard_random()
    true_guarded = [bool(scan.model(n).guarded_starts(n)) for n in lens]
    zsizes, k = sm.GUARD_ZERO[0]
    zlens = sm.guard_zero_lengths(zsizes, k)
    zscan = sm.zeros_scan(zsizes, max(zlens))
    true_zguarded = [bool(zscan.model(n).guarded_starts(n)) for n in zlens]
    lane_over = sm.budget_cases()[f"lane_{sm.LANE_HITS + 1}"]
    block_over = sm.budget_cases()[f"block_{sm.BLOCK_REC_CAP + 1}"]

    monkeypatch.setattr(sm, "WARM", 1 << 16)              # a record shifts (the first 64 KiB have none)
    assert _readout(sizes, "random") != true_regions
    monkeypatch.undo()
    monkeypatch.setattr(sm, "REGION_SPAN", 52 + sm.BLOCK_BYTES)   # where a truncated result is known
    assert _readout(sizes, "random") != true_regions
    monkeypatch.undo()
    monkeypatch.setattr(sm, "TRUNC_NONE", 61)             # a truncated result
    assert _readout(sizes, "random") != true_regions
    monkeypatch.undo()
    monkeypatch.setattr(sm, "GUARD_SPAN", 48)             # the guarded-branch predicate
    assert [bool(scan.model(n).guarded_starts(n)) for n in lens] != true_guarded
    assert [bool(zscan.model(n).guarded_starts(n)) for n in zlens] != true_zguarded
    monkeypatch.undo()
    monkeypatch.setattr(sm, "LANE_HITS", sm.LANE_HITS + 1)
    assert lane_over.model().record_fallback() is None
    monkeypatch.undo()
    monkeypatch.setattr(sm, "BLOCK_REC_CAP", sm.BLOCK_REC_CAP + 1)
    assert block_over.model().record_fallback() is None
    monkeypatch.undo()
    assert _readout(sizes, "random") == true_regions


def test_first_difference_names_the_block_and_the_stage():
    sizes = sm.SCAN_SETS[0]
    m = sm.scan_of(sizes, "random").model()
    counts = m.block_counts()
    regions = np.zeros(m.blocks * sm.BLOCK_REC_CAP, dtype=np.uint64)
    for b in range(m.blocks):
        regions[b * sm.BLOCK_REC_CAP:b * sm.BLOCK_REC_CAP + int(counts[b])] = m.block_regions(b)
    assert sm.first_difference(m, counts, regions).startswith("scan stage right")
    bad = regions.copy()
    bad[3 * sm.BLOCK_REC_CAP + 1] = 0                     # a record that reads as empty
    assert "block 3 record 1: record differs" in sm.first_difference(m, counts, bad)
    bad = regions.copy()
    bad[2 * sm.BLOCK_REC_CAP] ^= np.uint64(1 << 32)
    assert "block 2 record 0: truncated result differs" in sm.first_difference(m, counts, bad)
    c2 = counts.copy()
    c2[5] += 1
    assert "block 5 published" in sm.first_difference(m, c2, regions)
