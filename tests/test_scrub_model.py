"""CPU suite of the scrub model (tests/scrub_model.py).  The model is checked
against a second restatement that follows the reference statement by statement
-- CopyScrubber / DumbScrubber (src/system/scrub.rs:85-129), retrieve
(src/system/storage.rs:141-157), the statistics and clears
(storage.rs:193-268, src/system/mod.rs:271-298) -- with containers as objects
and the folds written out, and the properties the device tests rely on."""
import itertools
import math

import numpy as np
import pytest

import oracle
import scrub_model as scm


# ---- the reference, statement by statement ------------------------------------------
class Container:
    """DataContainer (storage.rs:12-21): a Chunk or a TargetChunk."""

    def __init__(self, chunk):
        self.chunk, self.keys = chunk, None

    def make_target(self, keys):
        self.chunk, self.keys = None, keys


class RefStorage:
    def __init__(self):
        self.database, self.target_map, self.size_written = {}, {}, 0

    def write(self, data, chunks):
        for o, ln in chunks:
            b = data[int(o):int(o) + int(ln)].tobytes()
            if scm.sha(b) not in self.database:  # entry(key).or_insert(value)
                self.database[scm.sha(b)] = Container(b)
            self.size_written += len(b)

    def retrieve(self, request):  # storage.rs:141-157
        retrieved = [self.database[h] for h in request]
        out = []
        for container in retrieved:
            if container.keys is None:
                out.append(container.chunk)
            else:
                out.append(b"".join(self.target_map[k] for k in container.keys))
        return out

    def copy_scrub(self):  # scrub.rs:91-113
        processed_data = 0
        for h, container in self.database.items():
            if container.keys is None:
                self.target_map.setdefault(h, container.chunk)
                processed_data += len(container.chunk)
            container.make_target([h])
        return processed_data, 0

    def dumb_scrub(self):  # scrub.rs:122-128
        return 0, 0

    def total_cdc_size(self):  # storage.rs:193-200
        total = 0
        for container in self.database.values():
            total = total + len(container.chunk) if container.keys is None else total
        return total

    def cdc_dedup_ratio(self):  # storage.rs:203-205
        return scm.ratio(self.size_written, self.total_cdc_size())

    def average_chunk_size(self):  # storage.rs:208-221
        count, size = 0, 0
        for container in self.database.values():
            count, size = count + 1, size + (len(container.chunk) if container.keys is None else 0)
        return size // count

    def full_cdc_dedup_ratio(self):  # storage.rs:223-231
        return scm.ratio(self.size_written, self.total_cdc_size() + sum(32 for _ in self.database))

    def total_dedup_ratio(self):  # storage.rs:250-261
        return scm.ratio(self.size_written, self.total_cdc_size() + sum(len(v) for v in self.target_map.values()))

    def clear_database(self):  # storage.rs:238-241
        self.size_written = 0
        self.database.clear()

    def clear_database_full(self):  # storage.rs:264-268
        self.size_written = 0
        self.database.clear()
        self.target_map.clear()


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _compare(m, r):
    assert m.size_written == r.size_written
    assert set(m.base) == set(r.database)
    assert m.target == r.target_map
    for h in m.base:
        assert m.retrieve([h]) == r.retrieve([h])
        assert (m.base[h][0] == scm.TARGET) == (r.database[h].keys is not None)
    assert _same(m.cdc_dedup_ratio(), r.cdc_dedup_ratio())
    assert _same(m.full_cdc_dedup_ratio(), r.full_cdc_dedup_ratio())
    assert _same(m.total_dedup_ratio(), r.total_dedup_ratio())
    if m.base:
        assert m.average_chunk_size() == r.average_chunk_size()


def _data(n, seed):
    return np.frombuffer(oracle.splitmix64_bytes(n, seed), dtype=np.uint8)


def _dup_data():
    a, b = _data(32768, 1), _data(8192, 2)
    return np.concatenate([a, b, a[:16384], b])


def test_model_follows_the_reference_through_a_sequence():
    data = _dup_data()
    chunks = oracle.fixed(data.size, 4096)
    m, r = scm.Storage(), RefStorage()
    _compare(m, r)  # empty: every ratio is 0 / 0
    m.put(data, chunks), r.write(data, chunks)
    _compare(m, r)
    assert m.scrub_dumb().processed_data == r.dumb_scrub()[0] == 0
    _compare(m, r)
    assert m.scrub_copy().processed_data == r.copy_scrub()[0] == m.scrub_stats()["target_bytes"]
    _compare(m, r)
    more = _data(12288, 3)
    both = np.concatenate([data[:8192], more])
    m.put(both, oracle.fixed(both.size, 4096)), r.write(both, oracle.fixed(both.size, 4096))
    _compare(m, r)
    assert m.scrub_copy().processed_data == r.copy_scrub()[0] == more.size
    _compare(m, r)
    m.clear_database(), r.clear_database()
    _compare(m, r)
    m.clear_database_full(), r.clear_database_full()
    _compare(m, r)
    assert not m.target


def test_copy_moves_the_ratio_and_leaves_cdc_ratio_infinite():
    data = _dup_data()
    m = scm.Storage()
    m.put(data, oracle.fixed(data.size, 4096))
    before = m.cdc_dedup_ratio()
    assert before > 1
    meas = m.scrub_copy()
    assert meas.processed_data == sum(len(v) for v in m.target.values()) and meas.data_left == 0
    assert m.total_dedup_ratio() == before
    assert m.cdc_dedup_ratio() == math.inf
    assert m.average_chunk_size() == 0
    assert m.read(list(m.base))[0].size == sum(len(v) for v in m.target.values())


def test_second_scrub_processes_nothing():
    data = _dup_data()
    m = scm.Storage()
    m.put(data, oracle.fixed(data.size, 4096))
    assert m.scrub_copy().processed_data > 0
    snap = (dict(m.base), dict(m.target))
    assert m.scrub_copy().processed_data == 0
    assert m.scrub_rechunk(lambda b: oracle.fixed(len(b), 512)).processed_data == 0
    assert snap == (m.base, m.target)


def test_clear_database_rewrite_scrub_leaves_the_target_unchanged():
    data = _dup_data()
    fs = scm.FileSystem()
    h = fs.create("f")
    fs.append(h, data, oracle.fixed(data.size, 4096))
    fs.store.scrub_copy()
    target = dict(fs.store.target)
    fs.clear()
    assert not fs.store.base and not fs.files and fs.store.target == target and fs.store.size_written == 0
    with pytest.raises(scm.fm.ModelError):
        fs.read_complete(h)
    h = fs.create("f")
    fs.append(h, data, oracle.fixed(data.size, 4096))
    assert fs.store.scrub_copy().processed_data == sum(len(v) for v in target.values())
    assert fs.store.target == target
    assert (fs.read_complete(h) == data).all()
    fs.clear_file_system()
    assert not fs.store.base and not fs.store.target and not fs.files


def test_rechunk_of_permuted_blocks_keeps_eight_values():
    pool = [_data(512, 10 + i) for i in range(8)]
    orders = list(itertools.islice(itertools.permutations(range(8)), 0, 5040, 720))
    data = np.concatenate([pool[i] for order in orders for i in order])
    assert data.size == len(orders) * 4096
    m = scm.Storage()
    m.put(data, oracle.fixed(data.size, 4096))
    assert len(m.base) == len(orders)
    meas = m.scrub_rechunk(lambda b: oracle.fixed(len(b), 512))
    assert meas.processed_data == data.size and meas.data_left == 0
    assert len(m.target) == 8 and set(m.target.values()) == {p.tobytes() for p in pool}
    assert all(kind == scm.TARGET and len(keys) == 8 for kind, keys in m.base.values())
    assert (m.read(list(m.base))[0] == data).all()  # dicts keep insertion order
    assert m.total_dedup_ratio() == data.size / 4096


def test_rechunk_shapes_and_writes_after_a_scrub():
    m = scm.Storage()
    data = _data(1000, 5)
    m.put(data, np.array([[0, 0], [0, 100], [100, 900]], dtype=np.uint64))
    m.scrub_rechunk(lambda b: oracle.fixed(len(b), 512))
    it = m.iterator()
    assert it[scm.sha(b"")] == (scm.TARGET, 0, [])  # a length-0 chunk: a target with no keys
    assert [len(k) for _, _, k in it.values()] == [0, 1, 2]
    # a write whose digest exists as a target adds nothing; a new digest is chunk-kind
    _, new = m.put(data, np.array([[0, 100], [1, 99]], dtype=np.uint64))
    assert new.tolist() == [False, True]
    assert m.scrub_stats()["chunk_containers"] == 1 and m.total_cdc_size() == 99
    with pytest.raises(KeyError):
        m.retrieve([scm.sha(b"absent")])
    m.target.clear()
    with pytest.raises(KeyError):  # a missing key is NotFound
        m.retrieve([scm.sha(data[:100].tobytes())])
