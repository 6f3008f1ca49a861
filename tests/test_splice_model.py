"""CPU suite of the splice model (tests/splice_model.py): the windowed rule equals
the whole-tail rule, a spliced file equals the file a single write of the new
content makes, and -- as conditions on the inputs the GPU suite
(tests/test_gpu_splice.py) shares -- the cases reach the paths their names
promise, so that the GPU suite cannot pass by missing the hard ones."""
import numpy as np
import pytest

import files_model as fm
import splice_model as spm


def written(name, data=None, chunks=None):
    """A model layer holding one file written in one call with the named chunker."""
    if data is None:
        data, chunks = spm.base(name)
    elif chunks is None:
        chunks = spm.chunk(name, data)
    f = fm.Files()
    h = f.create("f")
    f.append(h, data, chunks)
    return f, h


def both(name, data, chunks, offset, rem, ins):
    """The edit by windows and by the whole tail: the windowed stats and the table,
    after asserting that the two agree and that the file is its one-call twin."""
    fw, hw = written(name, data, chunks)
    ft, ht = written(name, data, chunks)
    sw = spm.splice(fw, hw, name, offset, rem, ins, windowed=True)
    st = spm.splice(ft, ht, name, offset, rem, ins, windowed=False)
    for k in ("first_span", "spans_removed", "spans_inserted", "resync_offset", "size_before", "size_after",
              "bytes_new"):
        assert sw[k] == st[k], (k, sw, st)
    assert spm.table(fw, hw) == spm.table(ft, ht)
    content = fw.read_complete(hw)
    ins = ins if ins is not None else np.zeros(0, np.uint8)
    assert content.tobytes() == data[:offset].tobytes() + ins.tobytes() + data[offset + rem:].tobytes()
    assert spm.table(fw, hw) == spm.twin(name, content), "offsets and SHA-256 digests of the one-call twin"
    assert fw.store.stats() == ft.store.stats()
    return sw


@pytest.mark.parametrize("name", list(spm.CHUNKERS))
def test_random_cases_windowed_equals_whole_tail_and_the_twin(name):
    data, chunks = spm.base(name)
    assert 200 < len(chunks), "hundreds of spans"
    stats = {}
    for label, offset, rem, ins in spm.random_cases(name):
        o_last = int(chunks[-1][0])
        where = label.rsplit("_", 1)[1]
        if where == "first":
            assert offset < int(chunks[0][1])
        elif where == "last":
            assert offset + max(rem, 1) > o_last and offset + rem <= data.size
        stats[label] = both(name, data, chunks, offset, rem, ins)
    early = [s for s in stats.values() if s["rounds"] == 1 and s["spans_removed"] >= 1]
    if name != "fixed":
        assert 2 * len(early) >= len(stats), "at least half resync in round 1"
        assert any(s["resync_offset"] < s["size_after"] for s in stats.values()), "one resyncs before the end"
    else:  # a fixed-size insert or delete of 1 byte never meets the old cuts again
        for label in ("insert1_first", "delete1_first"):
            assert stats[label]["rounds"] >= 3 and stats[label]["resync_offset"] == stats[label]["size_after"]
        assert stats["overwrite100_middle"]["rounds"] == 1
    for s in stats.values():
        assert s["window_bytes"] >= s["resync_offset"] - (spm.base(name)[1][s["first_span"]][0])


@pytest.mark.parametrize("name", ["fast", "ae", "fixed"])
def test_edges_land_where_their_names_say(name):
    data, chunks = spm.base(name)
    cases = spm.edge_cases(name)
    mid = len(chunks) // 2
    b = int(chunks[mid][0])
    got = {label: both(name, data, chunks, *case) for label, case in cases.items()}
    assert cases["at_boundary"][0] == b and got["at_boundary"]["first_span"] == mid - 1
    assert cases["boundary_plus_7"][0] - b == 7 and got["boundary_plus_7"]["first_span"] == mid - 1
    assert cases["boundary_plus_8"][0] - b == 8 and got["boundary_plus_8"]["first_span"] == mid
    assert cases["near_zero"][0] < 8 and got["near_zero"]["first_span"] == 0
    assert cases["append"][0] == data.size
    last = len(chunks) - 1
    assert got["append"]["first_span"] == (last if int(chunks[last][1]) >= 8 else last - 1)
    assert got["append"]["resync_offset"] == got["append"]["size_after"] == data.size + 300
    for label, size in (("truncate_to_0", 0), ("truncate_to_1", 1), ("truncate_to_boundary", b), ("delete_all", 0)):
        assert got[label]["size_after"] == size == got[label]["resync_offset"]
    assert got["truncate_to_0"]["spans_inserted"] == 0 and got["truncate_to_0"]["spans_removed"] == len(chunks)
    assert got["truncate_to_1"]["spans_inserted"] == 1
    # cut at a boundary: the span before it is chunked again (it may have read past its cut) and comes out equal
    assert got["truncate_to_boundary"]["first_span"] == mid - 1 and got["truncate_to_boundary"]["bytes_new"] == 0
    blk = cases["exact_block_at_0"][2]
    s = got["exact_block_at_0"]
    assert (s["first_span"], s["spans_removed"], s["resync_offset"]) == (0, 0, blk.size)
    assert s["spans_inserted"] >= 2 and s["rounds"] == 1


def test_splice_into_an_empty_file_equals_a_write():
    for name in spm.CHUNKERS:
        data = spm.rand(4001, 20000)
        f = fm.Files()
        h = f.create("f")
        s = spm.splice(f, h, name, 0, 0, data)
        assert spm.table(f, h) == spm.twin(name, data)
        assert (s["first_span"], s["spans_removed"], s["resync_offset"]) == (0, 0, data.size)


def test_round_cases_take_the_rounds_their_names_say():
    got = {}
    for label, (name, data, offset, rem, ins) in spm.round_cases().items():
        got[label] = both(name, data, spm.chunk(name, data), offset, rem, ins)
    for label in ("zeros_fast_insert_1", "fixed_insert_1"):
        assert got[label]["rounds"] >= 3 and got[label]["resync_offset"] == got[label]["size_after"], got[label]
    s = got["fixed_insert_512"]
    assert s["rounds"] == 1 and s["resync_offset"] == 41 * 512 and (s["spans_removed"], s["spans_inserted"]) == (1, 2)


def test_zero_length_spans_at_the_resync_offset_stay():
    """A file appended by hand with two spans of no bytes at the boundary where an
    edit two spans earlier resyncs: the first of the equal offsets is the one met."""
    name = "fast"
    data, chunks = spm.base(name, seed=5, n=32 << 10)
    i = 20
    offset = int(chunks[i][0]) + int(chunks[i][1]) // 2
    f, h = written(name, data, chunks)
    s = spm.splice(f, h, name, offset, 1, spm.rand(5001, 1))
    j = s["first_span"] + s["spans_removed"]  # the old boundary the overwrite resyncs at
    assert j < len(chunks) - 1
    holes = np.concatenate([chunks[:j], [[chunks[j][0], 0]] * 2, chunks[j:]])
    f, h = written(name, data, holes)
    s2 = spm.splice(f, h, name, offset, 1, spm.rand(5001, 1))
    assert s2["first_span"] + s2["spans_removed"] == j and s2["resync_offset"] == int(chunks[j][0])
    t = spm.table(f, h)
    k = s2["first_span"] + s2["spans_inserted"]
    assert [x[1] for x in t[k:k + 3]] == [0, 0, int(chunks[j][1])]


def test_window_policy_and_start_span():
    assert spm.window_end(10 ** 9, 1000, 10, 1024, 1) == 1010 + 4096 + 8
    assert spm.window_end(10 ** 9, 1000, 10, 1024, 3) == 1010 + 65536 + 8
    assert spm.window_end(2000, 1000, 10, 1024, 1) == 2000
    offs = [0, 100, 100, 100, 250, 400]
    assert [spm.start_span(offs, 5, x) for x in (0, 7, 8, 107, 108, 257, 258, 400)] == [0, 0, 0, 0, 3, 3, 4, 4]
    assert spm.start_span([0], 0, 0) == 0
