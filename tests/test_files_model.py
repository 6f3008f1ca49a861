"""CPU suite of the file-layer model (tests/files_model.py): it reproduces the
reference's recorded file-system answers (tests/golden/filesystem_known_answers.json,
from the reference's tests/filesystem.rs), and its segment read equals a direct
transcription of file_layer.rs:152-175 (skip_while / take_while) on files
written through one handle."""
import itertools
import json
import os

import numpy as np
import pytest

import files_model as fm
import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
KNOWN = json.load(open(os.path.join(HERE, "golden", "filesystem_known_answers.json")))


def _write(files, h, case_writes, size):
    whole = []
    for w in case_writes:
        data = np.full(w["len"], w["byte"], dtype=np.uint8)
        files.append(h, data, oracle.fixed(data.size, size))
        whole.append(data)
    return np.concatenate(whole)


def test_blocks_read_back_as_four_segments_then_empty():
    case = KNOWN["write_read_blocks"]
    files = fm.Files(seg_size=KNOWN["seg_size"])
    h = files.create("file")
    whole = _write(files, h, case["writes"], case["chunker"]["size"])
    assert whole.size == case["total"]
    r = files.open("file")
    got = [files.read(r) for _ in range(case["reads"])]
    assert [g.size for g in got] == case["read_lengths"]
    assert (np.concatenate(got) == whole).all()
    assert files.read(r).size == case["next_read_length"]


def test_small_file_reads_in_one_segment():
    case = KNOWN["small_file"]
    files = fm.Files(seg_size=KNOWN["seg_size"])
    whole = _write(files, files.create("file"), case["writes"], case["chunker"]["size"])
    r = files.open("file", readonly=case["readonly"])
    got = files.read(r)
    assert [got.size] == case["read_lengths"] and (got == whole).all()


def test_big_file_at_once():
    case = KNOWN["big_file_at_once"]
    files = fm.Files()
    _write(files, files.create("file"), case["writes"], case["chunker"]["size"])
    assert files.read_complete(files.open("file")).size == case["read_complete_length"]


def test_two_handles_on_one_file():
    case = KNOWN["two_handles"]
    files = fm.Files()
    h1 = files.create("file")
    h2 = files.open("file", readonly=True)
    _write(files, h1, case["writes"], 4096)
    assert files.read_complete(h2).size == case["read_complete_length"]


def test_readonly_and_name_rules():
    case = KNOWN["readonly_rules"]
    files = fm.Files()
    _write(files, files.create("file"), case["writes"], case["chunker"]["size"])
    ro = files.open("file", readonly=True)
    with pytest.raises(fm.ModelError) as ei:
        files.append(ro, np.ones(16, dtype=np.uint8), np.array([[0, 16]], dtype=np.uint64))
    assert ei.value.code == fm.EPERM and case["write_error"] == "PermissionDenied"
    got = files.read_complete(ro)
    assert got.size == case["read_complete_length"] and (got == case["read_complete_byte"]).all()
    assert files.read(ro).size == KNOWN["seg_size"]
    with pytest.raises(fm.ModelError) as ei:
        files.create("file", create_new=False)
    assert ei.value.code == fm.EEXIST
    with pytest.raises(fm.ModelError) as ei:
        files.open("nope")
    assert ei.value.code == fm.ENOTFOUND
    files.create("file", create_new=True)  # truncates
    assert files.read_complete(ro).size == 0


def test_dedup_ratios():
    case = KNOWN["dedup_ratio_fixed_4096"]
    files = fm.Files()
    h = files.create("file")
    for step in case["steps"]:
        data = np.full(step["len"], step["byte"], dtype=np.uint8)
        files.append(h, data, oracle.fixed(data.size, case["chunker"]["size"]))
        st = files.store.stats()
        assert st["bytes_written"] / st["unique_bytes"] == step["ratio"]


def _transcribed_read(spans, handle_offset, seg):
    """file_layer.rs:152-175 line by line; returns (hashes, new handle offset)."""
    bytes_read = 0

    def take(span):
        nonlocal bytes_read
        bytes_read += span.len
        if bytes_read > seg:
            bytes_read -= span.len
            return False
        return True

    hashes = [sp.hash for sp in itertools.takewhile(take, itertools.dropwhile(lambda sp: sp.offset < handle_offset,
                                                                                spans))]
    return hashes, handle_offset + bytes_read


SEG = 100
LENGTH_LISTS = {
    "plain": [30, 30, 30, 30, 30, 7],
    "exactly_the_segment": [40, 100, 60, 40, 1],
    "longer_than_the_segment_later": [50, 50, 101, 10],
    "longer_than_the_segment_first": [101, 10],
    "zero_lengths": [0, 0, 30, 0, 70, 0, 0, 100, 0, 5, 0],
    "only_zero_lengths": [0, 0, 0],
    "ones": [1] * 250,
}


@pytest.mark.parametrize("name", sorted(LENGTH_LISTS))
def test_segment_read_equals_the_transcription(name):
    lengths = LENGTH_LISTS[name]
    rng = np.random.default_rng(len(name))
    data = rng.integers(0, 256, max(sum(lengths), 1), dtype=np.uint8)
    files = fm.Files(seg_size=SEG)
    w = files.create("f")
    files.append_lengths(w, data, lengths)
    spans = files.files["f"]
    assert [sp.offset for sp in spans] == [sum(lengths[:i]) for i in range(len(lengths))]  # one handle: true offsets
    r = files.open("f", readonly=True)
    offset = 0
    for _ in range(len(lengths) + 2):
        want_hashes, want_offset = _transcribed_read(spans, offset, SEG)
        got = files.read(r)
        assert r.offset == want_offset
        assert got.tobytes() == b"".join(files.store.db[h] for h in want_hashes)
        assert got.tobytes() == data[offset:want_offset].tobytes()
        if want_offset == offset:  # the end of the file, or stuck on a span longer than the segment
            break
        offset = want_offset
    if name.startswith("longer_than_the_segment"):
        assert r.offset == sum(lengths[:lengths.index(101)]) < sum(lengths)  # stuck, as in the reference
    else:
        assert r.offset == sum(lengths)


def test_true_offsets_through_a_reopened_handle():
    """The stated deviation: a second handle appends at the file's end, so the
    segment reads still cover the whole file."""
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 300, dtype=np.uint8)
    files = fm.Files(seg_size=SEG)
    files.append_lengths(files.create("f"), data[:150], [50, 50, 50])
    files.append_lengths(files.open("f"), data[150:], [50, 50, 50])
    assert [sp.offset for sp in files.files["f"]] == [0, 50, 100, 150, 200, 250]
    r = files.open("f", readonly=True)
    got = np.concatenate([files.read(r) for _ in range(3)])
    assert (got == data).all() and files.read(r).size == 0


def test_distribution_drops_the_last_span_and_keeps_first_occurrence_order():
    data = np.frombuffer(b"aaaabbbbaaaaccccbbbbaaaa", dtype=np.uint8)
    files = fm.Files()
    h = files.create("f")
    files.append_lengths(h, data, [4] * 6)
    d = files.distribution(h)
    assert list(d.items()) == [(fm.sha(b"aaaa"), (2, 4)), (fm.sha(b"bbbb"), (2, 4)), (fm.sha(b"cccc"), (1, 4))]
    one = fm.Files()
    h = one.create("f")
    one.append_lengths(h, data, [24])
    assert one.distribution(h) == {}


def test_pread_clips():
    data = np.arange(200, dtype=np.uint8)
    files = fm.Files()
    h = files.create("f")
    files.append_lengths(h, data, [0, 7, 93, 0, 100])
    assert (files.pread(h, 5, 10) == data[5:15]).all()
    assert files.pread(h, 200, 10).size == 0 and files.pread(h, 3, 0).size == 0
    assert (files.pread(h, 190, 100) == data[190:]).all()
