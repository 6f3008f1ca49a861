"""CPU suite of the model of cdc_files_clone and cdc_files_diff_device
(tests/diff_model.py): on seeded random pairs of tables the exact model equals a
brute-force numpy mask over the two contents, the tables-only answer contains
the exact one, and every case of the GPU suite (tests/test_gpu_snapshot.py)
reaches the path it is named for -- the cases carry their own assertions, and
here they run on the model alone."""
import numpy as np
import pytest

import diff_model as dm
import files_model as fm
import gc_model as gm


def covers(outer, inner):
    """Every range of `inner` lies inside one of `outer`."""
    return all(any(o <= s and s + n <= o + m for o, m in outer) for s, n in inner)


def canonical(ranges):
    return all(n > 0 for _, n in ranges) and all(a + n < b for (a, n), (b, _) in zip(ranges, ranges[1:]))


def random_lengths(rng, n, style):
    """n span lengths of 0 .. 40 bytes; a third are 0, and by `style` the list
    starts with, ends with or holds runs of spans of length 0."""
    ln = rng.integers(1, 41, n)
    ln[rng.random(n) < 0.3] = 0
    if style == "zeros_first" and n:
        ln[:2] = 0
    if style == "zeros_last" and n:
        ln[-2:] = 0
    if style == "zero_runs" and n > 6:
        ln[3:6] = 0
    return ln


def recut(rng, lengths):
    """The same bytes cut again: spans merged, split, kept, and spans of length 0
    put at boundaries both lists have."""
    out, carry = [], 0
    for ln in lengths:
        ln = int(ln) + carry
        carry = 0
        kind = rng.integers(0, 6)
        if kind == 0 and ln > 1:
            cut = int(rng.integers(1, ln))
            out += [cut, ln - cut]
        elif kind == 1:
            carry = ln
        else:
            out.append(ln)
        if kind == 2:
            out.append(0)
    if carry:
        out.append(carry)
    return out


@pytest.mark.parametrize("seed", range(40))
def test_the_model_equals_a_mask_over_the_contents(seed):
    rng = np.random.default_rng(seed)
    style = ("plain", "zeros_first", "zeros_last", "zero_runs")[seed % 4]
    m = gm.Files()
    la = random_lengths(rng, int(rng.integers(0, 60)) if seed else 0, style)
    data = dm.rand(100 + seed, int(la.sum()))
    a = m.create("a")
    if len(la):
        m.append(a, data, dm.tiling(la))
    others = {}
    # b: the same bytes cut again, some flipped, the end grown or cut off; c: unrelated; e: empty
    lb = recut(rng, la)
    bdata = data.copy()
    if bdata.size:
        bdata[rng.random(bdata.size) < 0.05] ^= 0x11
    keep = int(rng.integers(0, len(lb) + 1)) if seed % 3 == 1 else len(lb)
    lb = lb[:keep]
    bdata = bdata[:sum(lb)]
    if seed % 3 == 2:
        extra = dm.rand(200 + seed, 30)
        lb, bdata = lb + [0, 30], np.concatenate([bdata, extra])
    for name, content, lengths in (("b", bdata, lb), ("c", dm.rand(300 + seed, 500), random_lengths(rng, 25, style)),
                                   ("e", data[:0], [])):
        h = m.create(name)
        lengths = np.asarray(lengths, dtype=np.int64)
        if name == "c":
            content = content[:int(lengths.sum())]
        if len(lengths):
            m.append(h, content, dm.tiling(lengths))
        others[name] = h
    dm.clone(m, "a", "a2")
    others["a2"] = m.open("a2")
    shared_seen = False
    for name, h in others.items():
        for x, y in ((a, h), (h, a)):
            exact, loose = dm.diff(m, x, y), dm.diff(m, x, y, tables_only=True)
            cx, cy = m.read_complete(x), m.read_complete(y)
            assert exact["ranges"] == dm.mask_ranges(cx, cy), name
            assert canonical(exact["ranges"]) and canonical(loose["ranges"])
            assert covers(loose["ranges"], exact["ranges"])
            assert exact["bytes_differing"] == sum(n for _, n in exact["ranges"])
            assert loose["bytes_differing"] == sum(n for _, n in loose["ranges"])
            assert exact["bytes_shared"] + exact["bytes_compared"] == min(cx.size, cy.size)
            assert loose["bytes_compared"] == 0 and loose["bytes_shared"] == exact["bytes_shared"]
            ps = dm.pieces(m._spans(x), m._spans(y))
            assert exact["pieces"] == len(ps) and (len(ps) == 0) == (min(cx.size, cy.size) == 0)
            assert all(e > s for s, e, *_ in ps) and [p[0] for p in ps[1:]] == [p[1] for p in ps[:-1]]
            shared_seen = shared_seen or exact["bytes_shared"] > 0
    assert dm.diff(m, a, others["a2"])["ranges"] == [] and dm.diff(m, a, others["a2"])["bytes_compared"] == 0
    assert shared_seen or data.size == 0


def test_tables_only_equals_exact_when_every_compared_byte_differs():
    m = gm.Files()
    data = dm.rand(1, 4000)
    a, b = m.create("a"), m.create("b")
    m.append(a, data, dm.tiling([1000, 1000, 1000, 1000]))
    other = data.copy()
    other[1000:2000] ^= 0xFF
    other[3000:3500] ^= 0xFF
    m.append(b, other, dm.tiling([1000, 1000, 1000, 500, 500]))
    exact, loose = dm.diff(m, a, b), dm.diff(m, a, b, tables_only=True)
    assert exact["ranges"] == [(1000, 1000), (3000, 500)]
    assert loose["ranges"] == [(1000, 1000), (3000, 1000)]  # [3500, 4000) is equal, but its span is another
    c = m.create("c")
    other[3500:] ^= 0xFF
    m.append(c, other, dm.tiling([1000, 1000, 1000, 500, 500]))
    assert dm.diff(m, a, c)["ranges"] == dm.diff(m, a, c, tables_only=True)["ranges"] == [(1000, 1000), (3000, 1000)]


def test_clone_is_deep_and_refuses_as_the_header_says():
    m = gm.Files()
    a = m.create("a")
    m.append(a, dm.rand(2, 300), dm.tiling([100, 0, 200]))
    before = dict(m.store.stats())
    assert dm.clone(m, "a", "b") == 3 and m.store.stats() == before
    m.files["b"][0].offset = 77
    assert m.files["a"][0].offset == 0
    for src, dst, code in (("nope", "x", fm.ENOTFOUND), ("a", "b", fm.EEXIST), ("a", "a", fm.EEXIST)):
        with pytest.raises(fm.ModelError) as e:
            dm.clone(m, src, dst)
        assert e.value.code == code
    m.create("empty")
    assert dm.clone(m, "empty", "empty2") == 0 and m.files["empty2"] == []


# ---- every case of the GPU suite reaches its path (the cases assert it themselves) --------------
def test_case_nothing_to_read():
    dm.case_nothing_to_read(dm.ModelDriver("fast"))


@pytest.mark.parametrize("tables_only", [False, True])
@pytest.mark.parametrize("n", [1, 4096])
def test_case_one_edit(n, tables_only):
    dm.case_one_edit(dm.ModelDriver("fast"), n, tables_only)


def test_case_edges_and_two_ranges_and_tail():
    out = dm.case_edges(dm.ModelDriver())
    assert len(out) == 30
    dm.case_two_ranges(dm.ModelDriver("fixed"))
    dm.case_tail(dm.ModelDriver())


def test_case_alignment_covers_every_head_tail_and_tile_count():
    seen = set()
    for L in dm.ALIGN_L:
        out = dm.case_alignment(dm.ModelDriver(), L)
        assert len(out) == 2 * min(17, L)
        for k in range(1, min(17, L) + 1):
            # the second piece: A's side starts k bytes into its container, B's at one's start; the tiles are
            # aligned on the second handle's side, so diff(b, a) cuts them k % 16 bytes before the piece
            seen.add((k % 16, (L - k) % 16, -(-(k % 16 + L - k) // dm.TILE)))
    assert {k for k, _, _ in seen} == set(range(16)) and {t for _, t, _ in seen} == set(range(16))
    assert {n for _, _, n in seen} >= {0, 1, 2, 3}


@pytest.mark.parametrize("tables_only", [False, True])
def test_case_same_slot_shifted(tables_only):
    dm.case_same_slot_shifted(dm.ModelDriver(), tables_only)


def test_case_dense():
    out = dm.case_dense(dm.ModelDriver())
    assert out["every_second"]["n_ranges"] == 8192 > 4096 and out["words"]["ranges"][4][1] > dm.TILE


@pytest.mark.parametrize("n", list(dm.COUNT_CASES))
def test_case_counts(n):
    out = dm.case_counts(dm.ModelDriver(), n)
    assert out["moved"]["pieces"] == 2 * n and out["moved"]["n_ranges"] == dm.COUNT_CASES[n]


def test_the_count_cases_cross_both_scan_blocks():
    pieces = sorted(2 * n for n in dm.COUNT_CASES) + sorted(dm.COUNT_CASES)
    ranges = sorted(dm.COUNT_CASES.values())
    for edge in (2048, 4096):
        assert any(p < edge for p in pieces) and edge in pieces and any(p > edge for p in pieces)
        assert any(r < edge for r in ranges) and edge in ranges and any(r > edge for r in ranges)
    assert {2047, 2048, 2049} <= set(dm.COUNT_CASES) and max(dm.COUNT_CASES) >= 5000


@pytest.mark.parametrize("tables_only", [False, True])
def test_case_insert(tables_only):
    for k in (1, 16, 17):
        dm.case_insert(dm.ModelDriver("fast"), k, tables_only)
