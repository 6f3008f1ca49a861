"""CPU suite of the bench fixture's model (tests/bench_model.py) and of the
plain data in chunkfs_amd/bench.py: the closed form the device uses for
get_to_dedup_ratio against the line-by-line transcription of
src/system/file_layer.rs:212-268, the refusals, the derived file on
files_model.Files, the size distribution, verify, and Throughput's integer-MB
division (src/bench/report.rs:167-176).  No device is needed."""
import math

import numpy as np
import pytest

import bench_model as bm
import files_model as fm

RATIOS = [1.0, 1.005, 1.5, 2.0, 3.99, 4.0, 7.3, 25.0]


def _random_unique(rng):
    """A unique list as unique_spans leaves it: [(index, length)], lengths 0..100 with many zeros."""
    u = int(rng.integers(0, 13))
    lengths = rng.integers(0, 101, size=u)
    lengths[rng.random(u) < 0.3] = 0
    return [(i, int(ln)) for i, ln in enumerate(lengths)]


def test_closed_form_equals_the_transcription():
    rng = np.random.default_rng(2024)
    checked = refused = 0
    for _ in range(4000):
        unique = _random_unique(rng)
        lengths = [ln for _, ln in unique]
        for ratio in RATIOS:
            if bm.never_ends(lengths, ratio):
                refused += 1
                for fn, arg in ((bm.transcription, unique), (bm.closed_form, lengths)):
                    with pytest.raises(fm.ModelError) as ei:
                        fn(arg, ratio)
                    assert ei.value.code == bm.EINVAL
                continue
            assert bm.transcription(unique, ratio) == bm.closed_form(lengths, ratio), (lengths, ratio)
            checked += 1
    assert checked > 20000 and refused > 100  # both sides of the refusal were exercised


def test_zero_length_entry_at_the_cycle_wrap_is_taken():
    # total = 20, one cycle is 10 bytes: two cycles, then the leading empty entry of the third.
    lengths = [0, 4, 6]
    assert bm.sizes(lengths, 2.0) == (20, 2)  # R = ceil(3 / 2) = 2: the cycle is [0, 4]
    lengths = [0, 10, 7]
    total, r = bm.sizes(lengths, 1.5)
    assert (total, r) == (25, 2)
    got = bm.closed_form(lengths, 1.5)
    assert got == [0, 1, 0, 1, 0, 2]  # 10, 20, then the empty entry; 30 > 25 ends the take; entry 2 remains
    assert got == bm.transcription(list(enumerate(lengths)), 1.5)


def test_ratio_one_is_one_exact_cycle():
    lengths = [5, 9, 1, 30]
    assert bm.closed_form(lengths, 1.0) == [0, 1, 2, 3]
    assert bm.closed_form([], 1.0) == []


def test_non_terminating_cycle_is_detected_not_run():
    assert bm.never_ends([0, 0, 5], 2.0)       # R = 2: both repeating entries are empty
    assert not bm.never_ends([0, 0, 5], 1.0)   # R = 3 reaches the 5
    assert not bm.never_ends([], 3.0)          # nothing to cycle over: the reference returns at once
    with pytest.raises(fm.ModelError):
        bm.transcription([(0, 0), (1, 0), (2, 5)], 2.0)


def test_as_usize_saturates_like_rust():
    assert bm.as_usize(float("nan")) == 0 and bm.as_usize(-1.5) == 0
    assert bm.as_usize(1e30) == bm.U64_MAX and bm.as_usize(7.99) == 7


def test_name_formatting_on_non_tie_ratios():
    # Exact decimal ties (x.xx5 representable in binary, e.g. 1.125) are left out: C's %.2f and Rust's {:.2}
    # are believed to agree on them but that cannot be pinned without a Rust toolchain.
    want = {1.0: "a.1.00", 1.005: "a.1.00", 1.5: "a.1.50", 2.0: "a.2.00", 3.99: "a.3.99", 4.0: "a.4.00",
            7.3: "a.7.30", 25.0: "a.25.00", 1.0 / 3.0: "a.0.33", 1234.5678: "a.1234.57"}
    for ratio, name in want.items():
        assert bm.name_of("a", ratio) == name
    assert bm.name_of("a.2.00", 1.5) == "a.2.00.1.50"


def _file(files, name, lengths, dup=()):
    """A file of len(lengths) spans with distinct contents, except that span j repeats span i for (i, j) in dup."""
    h = files.create(name)
    parts = [np.full(ln, 1 + i, dtype=np.uint8) for i, ln in enumerate(lengths)]
    for i, j in dup:
        parts[j] = parts[i].copy()
    data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    files.append_lengths(h, data, [p.size for p in parts])
    return h


def test_derived_file_on_the_model():
    files = fm.Files()
    _file(files, "a", [10, 20, 10, 30, 5, 7], dup=[(0, 2)])
    # spans 0..4 (the last is dropped), span 2 repeats span 0: unique = [10, 20, 30, 5]
    name = bm.get_to_dedup_ratio(files, "a", 2.0)
    assert name == "a.2.00" and files.exists(name)
    h = files.open(name, readonly=True)
    spans = files._spans(h)
    assert [sp.len for sp in spans] == [10, 20] * 4 + [10, 30, 5]  # 130 / 30: 4 cycles, 10 left: one more span
    assert [sp.offset for sp in spans] == list(np.cumsum([0] + [sp.len for sp in spans[:-1]]))
    assert files.size(h) == 165 and files.read_complete(h).size == 165
    # a second call replaces the file; a call on the derived file derives again
    assert bm.get_to_dedup_ratio(files, "a", 2.0) == name and len(files._spans(h)) == 11
    again = bm.get_to_dedup_ratio(files, name, 1.5)
    assert again == "a.2.00.1.50" and files.list() == ["a", "a.2.00", "a.2.00.1.50"]


def test_empty_and_refused_cases_on_the_model():
    files = fm.Files()
    files.create("none")
    _file(files, "one", [9])
    for name in ("none", "one"):  # 0 or 1 spans: U = 0
        new = bm.get_to_dedup_ratio(files, name, 3.0)
        assert files._spans(files.open(new)) == []
    before = files.list()
    for ratio in (0.99, float("nan"), float("inf"), -2.0):
        with pytest.raises(fm.ModelError) as ei:
            bm.get_to_dedup_ratio(files, "one", ratio)
        assert ei.value.code == bm.EINVAL
    with pytest.raises(fm.ModelError) as ei:
        bm.get_to_dedup_ratio(files, "missing", 2.0)
    assert ei.value.code == fm.ENOTFOUND
    _file(files, "hollow", [0, 0, 8, 3])  # unique = [0 bytes, 8]: the empty chunk repeats, R = 1 holds no byte
    with pytest.raises(fm.ModelError) as ei:
        bm.get_to_dedup_ratio(files, "hollow", 2.0)
    assert ei.value.code == bm.EINVAL
    assert files.list() == sorted(before + ["hollow"])  # a refused call changes nothing


def test_size_distribution_model():
    lengths = [0, 1, 999, 1000, 1001, 4096, 8191]
    assert bm.size_distribution(lengths, 1) == {ln: 1 for ln in lengths}
    assert bm.size_distribution(lengths, 1000) == {0: 3, 1000: 2, 4000: 1, 8000: 1}
    assert bm.size_distribution(lengths, 8192) == {0: 7}
    assert bm.size_distribution([], 7) == {}
    with pytest.raises(fm.ModelError):
        bm.size_distribution(lengths, 0)


def test_verify_model():
    a = np.arange(100, dtype=np.uint8)
    assert bm.verify(a, a.copy()) == (True, None)
    b = a.copy()
    b[[40, 70]] ^= 1
    assert bm.verify(a, b) == (False, 40)
    assert bm.verify(a, a[:99]) == (False, 99) and bm.verify(a[:99], a) == (False, 99)
    assert bm.verify(a[:0], a[:0]) == (True, None)


def test_throughput_divides_whole_megabytes():
    from chunkfs_amd import MB
    from chunkfs_amd.bench import Throughput, TimeMeasurement
    m = TimeMeasurement(write_time=2.0, read_time=0.5, chunk_time=1.0, hash_time=4.0)
    t = Throughput(3 * MB + MB - 1, m)  # (size / MB) is 3, not 3.99...
    assert (t.write, t.read, t.chunk, t.hash) == (1.5, 6.0, 3.0, 0.75)
    t = Throughput(MB - 1, m)  # under one MB rates 0
    assert (t.write, t.read, t.chunk, t.hash) == (0.0, 0.0, 0.0, 0.0)
    z = Throughput(2 * MB, TimeMeasurement())  # f64 division by a zero time
    assert z.write == math.inf and math.isnan(Throughput(0, TimeMeasurement()).read)


def test_time_measurement_adds_field_by_field():
    from chunkfs_amd.bench import TimeMeasurement
    a, b = TimeMeasurement(1, 2, 3, 4), TimeMeasurement(10, 20, 30, 40)
    s = a + b
    assert (s.write_time, s.read_time, s.chunk_time, s.hash_time) == (11, 22, 33, 44)
    t = sum([a, b, a])
    assert (t.write_time, t.hash_time) == (12, 48)


def test_measure_result_has_the_references_twelve_fields():
    from chunkfs_amd.bench import MeasureResult
    assert sorted(MeasureResult.__slots__) == sorted(
        ["date", "name", "chunker", "size", "dedup_ratio", "full_dedup_ratio", "avg_chunk_size", "chunk_count",
         "measurement", "throughput", "file_name", "path"])
