"""The reference's bench fixture (src/bench/mod.rs) and the plain data of its
report (src/bench/report.rs), over the device FileSystem.

CDCFixture measures a dataset with a chunker, verifies what was written and
reads the chunk-size distribution, as the reference's CLI, examples and
criterion benches do through it.  The work stays on the GPU: the dataset is
uploaded once per write, verification compares the file with the dataset in HBM
(cdc_file_verify_device) in place of the reference's loop over read_from_file
segments, and the size distribution is a device histogram.

Not mirrored: MeasureResult::write_to_csv, the fio dataset generator
(bench/generator.rs) and the CLI.
"""
import datetime
import os
import time
import uuid

from . import FileSystem, MB
from ._lib import check, lib


class VerifyError(ValueError):
    """io::ErrorKind::InvalidData of CDCFixture::verify (bench/mod.rs:248-271).
    first_diff: the smallest differing byte offset (None for a size mismatch)."""

    def __init__(self, msg, first_diff=None):
        super().__init__(msg)
        self.first_diff = first_diff


class Dataset:
    """Dataset (bench/mod.rs:20-52): a file on disk with a custom name; `size`
    is read once, here."""

    def __init__(self, path, name):
        self.path, self.name = str(path), str(name)
        self.size = os.stat(self.path).st_size

    def open(self):
        return open(self.path, "rb")


class TimeMeasurement:
    """TimeMeasurement (report.rs:113-157): seconds; `+` adds field by field."""

    __slots__ = ("write_time", "read_time", "chunk_time", "hash_time")

    def __init__(self, write_time=0.0, read_time=0.0, chunk_time=0.0, hash_time=0.0):
        self.write_time, self.read_time = float(write_time), float(read_time)
        self.chunk_time, self.hash_time = float(chunk_time), float(hash_time)

    def __add__(self, rhs):
        return TimeMeasurement(self.write_time + rhs.write_time, self.read_time + rhs.read_time,
                               self.chunk_time + rhs.chunk_time, self.hash_time + rhs.hash_time)

    def __radd__(self, lhs):  # sum() starts from 0, as Sum starts from default()
        return self if lhs == 0 else NotImplemented

    def __repr__(self):
        return (f"Read time: {self.read_time}s\nWrite time: {self.write_time}s\n"
                f"Chunk time: {self.chunk_time}s\nHash time: {self.hash_time}s")


def _rate(whole_mb, seconds):
    """f64 division: inf for a zero time, nan for 0 / 0."""
    if seconds:
        return whole_mb / seconds
    return float("inf") if whole_mb else float("nan")


class Throughput:
    """Throughput::new (report.rs:167-176): MB/s, with the reference's integer
    division -- (size / MB) as f64 / seconds -- so a dataset under 1 MB rates 0."""

    __slots__ = ("chunk", "hash", "write", "read")

    def __init__(self, size, measurement):
        whole = int(size) // MB
        self.chunk, self.hash = _rate(whole, measurement.chunk_time), _rate(whole, measurement.hash_time)
        self.write, self.read = _rate(whole, measurement.write_time), _rate(whole, measurement.read_time)

    def __str__(self):
        return (f"Chunk throughput: {self.chunk:.3f} MB/s\nHash throughput: {self.hash:.3f} MB/s\n"
                f"Write throughput: {self.write:.3f} MB/s\nRead throughput: {self.read:.3f} MB/s")


class MeasureResult:
    """MeasureResult (report.rs:11-25), its twelve fields."""

    __slots__ = ("date", "name", "chunker", "size", "dedup_ratio", "full_dedup_ratio", "avg_chunk_size",
                 "chunk_count", "measurement", "throughput", "file_name", "path")

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields[k])

    def __repr__(self):
        return f"Dataset: {self.name}\n{self.measurement!r}\nDedup ratio: {self.dedup_ratio:.3f}"


class DedupMeasurement:
    """DedupMeasurement (report.rs:191-195)."""

    __slots__ = ("name", "dedup_ratio")

    def __init__(self, name, dedup_ratio):
        self.name, self.dedup_ratio = name, dedup_ratio

    def __repr__(self):
        return f"DedupMeasurement {{ name: {self.name!r}, dedup_ratio: {self.dedup_ratio} }}"


class CDCFixture:
    """CDCFixture (bench/mod.rs:54-283) over a device FileSystem: `fs`, or one
    created from **fs_kwargs (max_chunks, arena_bytes, hash, ...).  A dataset is
    written with one write_to_file, so it must fit in HBM beside the store, the
    buffer it is read back into and -- during verify -- a second copy of it."""

    def __init__(self, fs=None, **fs_kwargs):
        self.fs = fs if fs is not None else FileSystem(**fs_kwargs)

    def _init_file(self, chunker):
        name = str(uuid.uuid4())
        return self.fs.create_file(name, chunker), name

    def fill_with(self, data, chunker):
        """Fills the store with the bytes of `data` (an object with read())."""
        handle, _ = self._init_file(chunker)
        self.fs.write_from_stream(handle, data)
        self.fs.close_file(handle)

    def fill_with_many(self, datas, chunker):
        """Fills the store with every one of `datas` (host bytes or CUDA uint8
        tensors), each in a file of its own, by ONE write_to_files; returns the
        files' names in the order of `datas`."""
        made = [self._init_file(chunker) for _ in datas]
        self.fs.write_to_files([h for h, _ in made], datas)
        for h, _ in made:
            self.fs.close_file(h)
        return [name for _, name in made]

    def measure(self, dataset, chunker):
        """One measurement of `dataset` with `chunker` (bench/mod.rs:93-140)."""
        chunker_name = repr(chunker)
        handle, name = self._init_file(chunker)
        with dataset.open() as f:
            t0 = time.perf_counter()
            self.fs.write_from_stream(handle, f)
            write_time = time.perf_counter() - t0
        wm = self.fs.close_file(handle)
        read_time = self.verify(dataset, name)
        measurement = TimeMeasurement(write_time, read_time, wm["chunk_time"], wm["hash_time"])
        return MeasureResult(
            date=datetime.datetime.now(datetime.timezone.utc), name=dataset.name, file_name=name,
            chunker=chunker_name, measurement=measurement, throughput=Throughput(dataset.size, measurement),
            dedup_ratio=self.fs.cdc_dedup_ratio(), full_dedup_ratio=self.fs.full_cdc_dedup_ratio(),
            avg_chunk_size=self.fs.average_chunk_size(), size=dataset.size, path=dataset.path,
            chunk_count=self.chunk_count())

    def measure_multi(self, dataset, chunker, n):
        """n measurements; the database is cleared before the first run and
        after each one (bench/mod.rs:145-164)."""
        self.fs.clear_database()
        out = []
        for _ in range(n):
            self.fs.clear_database()
            out.append(self.measure(dataset, chunker))
        return out

    def measure_repeated(self, dataset, chunker, m):
        """m measurements; the database is cleared before the first run only
        (bench/mod.rs:170-186)."""
        self.fs.clear_database()
        return [self.measure(dataset, chunker) for _ in range(m)]

    def dedup_ratio(self, dataset, chunker):
        """The dedup ratio of `dataset` under `chunker`; clears the database on
        call (bench/mod.rs:191-210)."""
        self.fs.clear_database()
        handle, name = self._init_file(chunker)
        with dataset.open() as f:
            self.fs.write_from_stream(handle, f)
        self.fs.close_file(handle)
        self.verify(dataset, name)
        return DedupMeasurement(dataset.name, self.fs.cdc_dedup_ratio())

    def size_distribution(self, adjustment):
        """{chunk length // adjustment * adjustment: count} over the store
        (bench/mod.rs:218-232); does not clear the database."""
        return self.fs.store.size_distribution(adjustment)

    def chunk_count(self):
        """storage_iterator().count() (bench/mod.rs:234-236)."""
        return check(lib().cdc_store_iterate_device(self.fs.store._h, None, None, None, None, 0, None))

    def verify(self, dataset, name):
        """CDCFixture::verify (bench/mod.rs:241-275): returns the seconds one
        read_file_complete of file `name` took (into a device buffer); raises
        VerifyError when the file's size or contents differ from the dataset.
        The contents are compared on the device against the uploaded dataset,
        in place of the reference's loop over read_from_file segments."""
        import torch
        dev = f"cuda:{self.fs.device}"
        handle = self.fs.open_file_readonly(name)
        try:
            size = self.fs.stat(handle)["size"]
            out = torch.empty(max(size, 1), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            got = self.fs.read_complete_device(handle, out.data_ptr(), size)
            read_time = time.perf_counter() - t0
            del out
            if got != dataset.size:
                raise VerifyError("dataset size and size of written file are different")
            with dataset.open() as f:
                raw = f.read()
            if len(raw) != dataset.size:
                raise VerifyError("dataset size and size of written file are different")
            if raw:
                data = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
                torch.cuda.synchronize(dev)
                same, diff = self.fs.verify_device(handle, data.data_ptr(), len(raw))
            else:
                same, diff = self.fs.verify_device(handle, None, 0)
            if not same:
                raise VerifyError(f"contents of dataset and written file are different (first at byte {diff})", diff)
            return read_time
        finally:
            handle._close()
