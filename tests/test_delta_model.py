"""CPU suite of the delta's model (tests/delta_model.py): every case on the model
alone.  ModelDriver.delta checks each answer against the two contents -- the ops
tile [0, size_b), rebuild B from A, are canonical, and every COPY edge next to a
LITERAL is maximal -- and the cases assert that they reach the path they are
named for.  The GPU suite (tests/test_gpu_delta.py) runs the same cases on the
device layer beside the model."""
import numpy as np
import pytest

import delta_model as dl

LIT = dl.LIT


def test_the_prototype_table_holds():
    out = dl.case_prototype(dl.ModelDriver("fixed"))
    assert out["overwrite"]["bytes_literal_tables"] == 512 and out["overwrite"]["regions"] == 1
    assert out["zeros"]["spans_matched"] == 9 and out["swapped"]["spans_matched"] == 8


@pytest.mark.parametrize("name", ["fixed", "fast"])
def test_insert_at_offset_0(name):
    for k in range(1, 18):
        r = dl.case_insert(dl.ModelDriver(name), k)["insert"]
        assert r["n_ops"] == 2 and r["bytes_literal"] == k and r["bytes_literal_tables"] >= k
    r = dl.case_insert(dl.ModelDriver(name), 5, True)["insert"]
    assert r["bytes_literal"] == r["bytes_literal_tables"]
    assert (r["spans_matched"] == 0) == (name == "fixed") and r["regions"] == 1


@pytest.mark.parametrize("tables_only", [False, True])
def test_edits_in_the_middle(tables_only):
    out = dl.case_edits(dl.ModelDriver("fast"), tables_only)
    for r in out.values():
        assert r["spans_matched"] > 0 and 0 < r["bytes_literal_tables"] < 8 * 1024  # a few spans around each edit


@pytest.mark.parametrize("L", dl.ALIGN_L)
def test_alignment(L):
    out = dl.case_alignment(dl.ModelDriver(), L)
    assert any(r["n_ops"] == 1 for r in out.values()) or L == 1  # the region that vanishes
    dl.case_misalign(dl.ModelDriver(), L)


def test_positions_sit_on_the_tile_edges():
    assert dl.align_positions(17) == [0, 16, None]
    assert dl.align_positions(8193) == [0, 1, 4095, 4096, 4097, 8191, 8192, None]
    assert dl.align_positions(4097) == [0, 1, 4095, 4096, None]


def test_overlap_nearest_empty_spans_and_degenerate():
    d = dl.ModelDriver()
    out = dl.case_overlap(d)
    assert out["zeros"]["ops"] == [(0, 812, 0), (812, 512, 512)]  # forward took the whole region
    out = dl.case_nearest(dl.ModelDriver())
    assert out["group"]["spans_matched"] == 2049
    dl.case_empty_spans(dl.ModelDriver())
    out = dl.case_degenerate(dl.ModelDriver())
    assert out["equal_sizes"]["spans_matched"] == 0 and out["unequal_sizes"]["regions"] == 1


@pytest.mark.parametrize("changed,lead", list(dl.COUNT_CASES))
def test_counts(changed, lead):
    out = dl.case_counts(dl.ModelDriver(), changed, lead)
    assert out["exact"]["n_ops"] == dl.COUNT_CASES[changed, lead]
    assert {2047, 2048, 2049} <= set(dl.COUNT_CASES.values()) and {2047, 2048, 2049} <= {c for c, _ in dl.COUNT_CASES}


def test_the_model_against_brute_force_on_random_tables():
    """Random contents over a small alphabet of chunks, random cuts: whatever
    the anchors say, the answer rebuilds B and is canonical and maximal."""
    rng = np.random.default_rng(7)
    blocks = [dl.rand(100 + i, int(rng.integers(1, 40))) for i in range(6)]
    for trial in range(60):
        d = dl.ModelDriver()
        pick = lambda: [blocks[i] for i in rng.integers(0, 6, int(rng.integers(0, 12)))]  # noqa: E731
        pa, pb = pick(), pick()
        cat = lambda p: np.concatenate(p) if p else dl.rand(1, 0)  # noqa: E731
        a = d.file("a", cat(pa), dl.tiling([x.size for x in pa]))
        b = d.file("b", cat(pb), dl.tiling([x.size for x in pb]))
        for t in (False, True):
            d.delta(a, b, t)
