"""GPU suite of removal and collection (include/chunkfs_amd.h, "Removal and
collection"): cdc_files_remove, cdc_files_collect and cdc_store_retain_device
against the model of tests/gc_model.py, bit for bit.  Every case is a few MB at
most.  After each collect: the collect's own stats (the move groups included)
against the model's planner, the store's stats, contains for every digest ever
written, and every read form of every surviving file."""
import os

import numpy as np
import pytest

import files_model as fm
import gc_model as gm
import store_model as sm
from test_gpu_files import Pair, _code, _digests, _tiling
from test_gpu_index_probing import Payloads, crafted, distinct_j, store_put_checked

pytestmark = pytest.mark.gpu
MB = 1 << 20
KNOB = "CHUNKFS_AMD_GC_BOUNCE"


@pytest.fixture(autouse=True)
def _no_knob():
    old = os.environ.pop(KNOB, None)
    yield
    os.environ.pop(KNOB, None)
    if old is not None:
        os.environ[KNOB] = old


def contains(store, digests):
    """contains_device of host digests -> list of 0/1."""
    import torch
    dig = np.ascontiguousarray(np.asarray(digests, dtype=np.uint8)).reshape(-1, 32)
    if not len(dig):
        return []
    dd = sm.dev(dig)
    found = torch.full((len(dig),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = store.contains_device(dd.data_ptr(), len(dig), found.data_ptr())
    out = found.cpu().numpy().tolist()
    assert n == sum(out)
    return out


class GcPair(Pair):
    """The device layer and gc_model.Files, driven side by side."""

    def __init__(self, c, seg=8192, max_chunks=1 << 12, arena=8 * MB, fs=None):
        super().__init__(c, seg=seg, max_chunks=max_chunks, arena=arena)
        if fs is not None:
            self.fs = fs
        self.m = gm.Files(seg_size=seg)
        self.seen = set()  # every digest ever written
        self.open_files = {}

    def file(self, name):
        if name not in self.open_files:
            self.open_files[name] = self.create(name)
        return self.open_files[name]

    def append(self, hm, data, chunks):
        super().append(hm, data, chunks)
        self.seen.update(bytes(d) for d in _digests(data, np.asarray(chunks, dtype=np.uint64).reshape(-1, 2)))

    def remove(self, name):
        self.fs.remove_file(name)
        self.m.remove(name)
        return self.open_files.pop(name)

    def collect(self, w=None):
        if w is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = str(w)
        got = self.fs.collect()
        want = self.m.collect(gm.DEFAULT_BOUNCE if w is None else w)
        assert {k: got[k] for k in want} == want
        assert got["seconds"] > 0
        return got

    def check_store(self):
        sm.assert_stats(self.fs.store, self.m.store)
        seen = sorted(self.seen)
        assert contains(self.fs.store, [np.frombuffer(k, np.uint8) for k in seen]) == \
            [int(k in self.m.store.db) for k in seen]

    def check_reads(self, name, full=True):
        import torch
        hm = self.open(name, readonly=True)
        want = self.check_file(hm, shift=5)  # stat, read_complete with spans, hashes
        if not full:
            return
        spans = self.m._spans(hm[1])
        edges = [s.offset for s in spans if 0 < s.offset < want.size]
        for e in edges[:2] + edges[-2:]:  # a pread across a span edge
            self.pread(hm, max(e - 7, 0), 40, shift=e % 16)
        self.pread(hm, 0, want.size + 3)
        for _ in range(64):  # the read_from_file loop
            if not self.read_segment(hm).size:
                break
        assert self.fs.chunk_count_distribution(hm[0]) == self.m.distribution(hm[1])
        d = sm.dev(want if want.size else np.zeros(1, np.uint8))
        assert self.fs.verify_device(hm[0], d.data_ptr(), want.size) == (True, None)
        if want.size:
            d[want.size // 2] ^= 1
            torch.cuda.synchronize()
            assert self.fs.verify_device(hm[0], d.data_ptr(), want.size) == (False, want.size // 2)

    def check_all(self):
        self.check_store()
        assert self.fs.list_files() == self.m.list()
        for name in self.m.list():
            self.check_reads(name)


def interleave(p, data, lengths, dead, keep="keep", gone="dead"):
    """Containers of `lengths`, tiling `data`, stored in this order: the ones
    whose index is in `dead` through file `gone`, the others through `keep`."""
    chunks = _tiling(lengths)
    p.file(keep), p.file(gone)
    for i, ch in enumerate(chunks):
        p.append(p.file(gone if i in dead else keep), data, [ch])


def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ---- which containers die -------------------------------------------------------------
LENGTHS = [100, 3000, 4097, 1, 2500, 16, 4096, 777, 15, 3333, 17, 2048]
DEAD = {"first": {0}, "last": {11}, "every_second": set(range(0, 12, 2)), "all_but_one": set(range(12)) - {5},
        "none": set(), "all": set(range(12))}


@pytest.mark.parametrize("which", list(DEAD))
def test_which_containers_die(which):
    import chunkfs_amd as c
    data = rand(1, sum(LENGTHS))
    p = GcPair(c)
    interleave(p, data, LENGTHS, DEAD[which])
    dead_handle = p.remove("dead")
    with pytest.raises(c.CdcError) as e:
        p.fs.stat(dead_handle[0])
    assert _code(e) == c._lib.CDC_ENOTFOUND
    r = p.collect()
    assert r["containers_after"] == 12 - len(DEAD[which])
    if which == "first":  # a gap of 112 bytes: the first survivor overlaps its own destination
        assert (r["groups_direct"], r["groups_bounced"]) == (0, 1) and r["bytes_moved"] == r["arena_used_after"]
    if which in ("none", "last"):
        assert r["bytes_moved"] == 0
    p.check_all()
    if which == "all":
        assert p.fs.store.stats()["arena_used"] == 0
    # a fresh write works, and a file of the removed name is a new, empty file
    again = p.create("dead")
    assert p.fs.stat(again[0])["size"] == 0 and p.fs.stat(dead_handle[0])["size"] == 0
    p.append(again, data, _tiling(LENGTHS)[3:9])
    p.append(p.file("keep"), data, [[50, 600]])
    p.check_all()


# ---- container lengths ----------------------------------------------------------------
@pytest.mark.parametrize("zero", ["kept_before_a_dead_one", "kept_after_a_dead_one", "dead"])
def test_container_lengths(zero):
    """0, 1, 15, 16, 17, 4095, 4096, 4097, each live and dead; the length-0
    container (there is one digest of no bytes) directly before or after a dead
    one, or dead itself."""
    import chunkfs_amd as c
    body = [1, 1, 15, 15, 16, 16, 17, 17, 4095, 4095, 4096, 4096, 4097, 4097]
    dead = set(range(0, len(body), 2))
    if zero == "kept_before_a_dead_one":
        lengths, dead = [0, 100] + body, {1} | {i + 2 for i in dead}
    elif zero == "kept_after_a_dead_one":
        lengths, dead = [100, 0] + body, {0} | {i + 2 for i in dead}
    else:
        lengths, dead = [100, 0] + body, {1} | {i + 2 for i in dead}
    p = GcPair(c)
    interleave(p, rand(2, sum(lengths)), lengths, dead)
    p.remove("dead")
    for w in (1, None):  # one container per bounced group, then the default
        r = p.collect(w)
        p.check_all()
    assert r["bytes_moved"] == 0
    assert fm.sha(b"") in p.seen and p.m.store.contains(fm.sha(b"")) == (zero != "dead")


# ---- groups and W -----------------------------------------------------------------------
def big_layer(c):
    """About 4 MiB in 420 containers of 1 .. 20 KiB; the first and every seventh
    are dead, so the gap starts at a few bytes and grows past any small W."""
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, 20000, 420).tolist()
    lengths[0] = 33
    dead = set(range(0, 420, 7))
    data = rand(4, sum(lengths))
    p = GcPair(c, max_chunks=1 << 10)
    chunks = _tiling(lengths)
    keep_a, keep_b, gone = p.file("a"), p.file("b"), p.file("dead")
    at = 0
    while at < 420:  # runs of up to 6 kept containers as one append, the dead one on its own
        if at in dead:
            p.append(gone, data, [chunks[at]])
            at += 1
        else:
            end = at
            while end < 420 and end not in dead and end - at < 6:
                end += 1
            p.append(keep_a if at % 2 else keep_b, data, chunks[at:end])
            at = end
    p.remove("dead")
    longest = max(sm.round_up16(n) for i, n in enumerate(lengths) if i not in dead)
    return p, longest


def test_groups_and_bounce_sizes():
    import chunkfs_amd as c
    outcomes = []
    for w in ("longest", "longest_and_one", 64 << 10, None):
        p, longest = big_layer(c)
        w = {"longest": longest, "longest_and_one": longest + 4096}.get(w, w)
        r = p.collect(w)  # the group counts equal the model planner's
        p.check_store()
        whole = {n: p.check_file(p.open(n, readonly=True)).tobytes() for n in p.m.list()}
        outcomes.append((r, p.fs.store.stats()["arena_used"], whole))
        if w is None:
            assert (r["groups_direct"], r["groups_bounced"]) == (0, 1)  # W = the bytes to move
            p.check_all()
        else:
            assert r["groups_bounced"] > 1 and r["groups_direct"] > 0, "bounced first, direct once the gap allows"
    assert len({(o[0]["groups_direct"], o[0]["groups_bounced"]) for o in outcomes}) > 2
    for o in outcomes[1:]:  # all runs leave identical stores
        assert o[1:] == outcomes[0][1:]
        assert o[0]["bytes_moved"] == outcomes[0][0]["bytes_moved"]


# ---- refcounts and the segmented passes -------------------------------------------------
def test_one_chunk_ten_thousand_times_and_a_shared_chunk():
    import chunkfs_amd as c
    data = rand(5, 4000)
    p = GcPair(c, max_chunks=1 << 14)  # a put is checked as if every chunk were new
    gone, many, kept = p.file("gone"), p.file("many"), p.file("kept")
    p.append(gone, data, [[0, 500], [500, 300]])        # [0, 500) dies; [500, 800) is shared with `kept`
    p.append(many, data, [[1000, 64]] * 10000)          # one slot, every lane of every wave
    p.append(kept, data, [[500, 300], [2000, 1000]])
    p.remove("gone")
    r = p.collect()
    assert (r["containers_before"], r["containers_after"]) == (4, 3)
    import ctypes
    split = (ctypes.c_double * 6)()
    assert c._lib.lib().cdc_debug_collect_split(split, 6) == 6  # the passes of the collect just done
    assert all(x > 0 for x in split) and sum(split) <= r["seconds"] * 1e3 * 1.01
    st = p.fs.store.stats()
    assert (st["chunks_written"], st["bytes_written"]) == (10002, 640000 + 1300)
    assert contains(p.fs.store, _digests(data, [[0, 500], [500, 300]])) == [0, 1]
    p.check_all()


def test_a_thousand_small_files_every_second_removed():
    import chunkfs_amd as c
    rng = np.random.default_rng(6)
    p = GcPair(c, max_chunks=1 << 12)
    ch = c.FSChunker(64)
    names = [f"f{i:04d}" for i in range(1000)]
    sizes = rng.integers(0, 4, 1000) * 64  # 0 .. 3 spans; empty files among them
    datas = [rand(1000 + i // 3, 192)[:n] for i, n in enumerate(sizes)]  # every block is shared by three files
    handles = [p.create(n, ch) for n in names]
    assert p.fs.write_to_files([h[0] for h in handles], datas) == (sizes // 64).tolist()
    for (h, mh), d in zip(handles, datas):
        p.m.append_lengths(mh, d, [64] * (d.size // 64))
        p.seen.update(p.m.hashes(mh))
    for n in names[::2]:
        p.fs.remove_file(n)
        p.m.remove(n)
    r = p.collect()
    assert 0 < r["containers_after"] < r["containers_before"]
    p.check_store()
    assert p.fs.list_files() == p.m.list()
    for k, n in enumerate(p.m.list()):
        p.check_reads(n, full=k % 50 == 0)


# ---- the index rebuild, through the bare store -------------------------------------------
def retain_checked(st, model, keep):
    """retain of host digests; the model does the same."""
    want = model.retain(keep)
    assert st.retain(keep) == want
    sm.assert_stats(st, model)


def everything_is_where_the_model_says(st, model, dig):
    assert contains(st, dig) == [int(bytes(d) in model.db) for d in dig]
    kept = [d for d in dig if bytes(d) in model.db]
    if kept:
        sm.get_checked(st, model, np.array(kept[::-1]))


def test_rebuild_of_a_cluster_that_wraps_past_the_last_slot():
    """300 digests at home in the last slot: one cluster across the table end.
    Every second one dies; the survivors must be found again and the dropped ones
    be absent although survivors lie further along the old probe sequence."""
    import chunkfs_amd as c
    rng = np.random.default_rng(31)
    dig = crafted(distinct_j(rng, 300), -1, rng)
    pay = Payloads(7, 700)
    d_data = sm.dev(pay.data)
    st, model = c.ChunkStore(512, 1 << 16), gm.Store()
    store_put_checked(st, model, d_data, pay.data, pay.take(300), dig)
    retain_checked(st, model, dig[1::2])
    everything_is_where_the_model_says(st, model, dig)
    # a dropped digest is new again (with other bytes than it first came with), a kept one is not
    store_put_checked(st, model, d_data, pay.data, pay.take(300), dig[rng.permutation(300)])
    assert st.stats()["unique_chunks"] == 300
    everything_is_where_the_model_says(st, model, dig)


@pytest.mark.parametrize("keep_first", [True, False])
def test_rebuild_of_a_pair_with_equal_first_eight_bytes(keep_first):
    """Two digests with one 64-bit key (the index's serial pass placed the
    second): one dies, the other is kept -- both ways round."""
    import chunkfs_amd as c
    rng = np.random.default_rng(32)
    pair = crafted(np.array([77, 77]), 5, rng)
    assert (pair[0, :8] == pair[1, :8]).all() and (pair[0] != pair[1]).any()
    others = crafted(distinct_j(rng, 20), 5, rng)
    dig = np.concatenate([others[:10], pair[:1], others[10:], pair[1:]])
    pay = Payloads(8, 100)
    d_data = sm.dev(pay.data)
    st, model = c.ChunkStore(64, 1 << 14), gm.Store()
    store_put_checked(st, model, d_data, pay.data, pay.take(len(dig)), dig)
    keep = np.concatenate([others[::3], pair[:1] if keep_first else pair[1:]])
    retain_checked(st, model, keep)
    everything_is_where_the_model_says(st, model, dig)
    store_put_checked(st, model, d_data, pay.data, pay.take(2), pair)  # the dropped one of the pair is new
    everything_is_where_the_model_says(st, model, dig)


def test_retain_with_duplicates_with_nothing_and_with_an_absent_digest():
    import chunkfs_amd as c
    rng = np.random.default_rng(33)
    dig = crafted(distinct_j(rng, 41), np.arange(41) * 3, rng)
    dig, absent = dig[:40], dig[40:]
    pay = Payloads(9, 100)
    d_data = sm.dev(pay.data)
    st, model = c.ChunkStore(64, 1 << 14), gm.Store()
    store_put_checked(st, model, d_data, pay.data, pay.take(40), dig)
    before = (st.stats(), sm.get_checked(st, model, dig).tolist())
    with pytest.raises(c.CdcError) as e:
        st.retain(np.concatenate([dig[:5], absent, dig[7:9]]))
    assert _code(e) == c._lib.CDC_ENOTFOUND
    assert (st.stats(), sm.get_checked(st, model, dig).tolist()) == before  # bit-identical: nothing changed
    retain_checked(st, model, np.concatenate([dig[30:35], dig[3:8], dig[30:33], dig[4:5]]))  # duplicates count
    assert st.stats()["chunks_written"] == 14 and st.stats()["unique_chunks"] == 10
    everything_is_where_the_model_says(st, model, dig)
    retain_checked(st, model, dig[:0])  # n = 0 keeps none
    assert st.stats()["arena_used"] == 0 and contains(st, dig) == [0] * 40
    store_put_checked(st, model, d_data, pay.data, pay.take(3), dig[:3])
    everything_is_where_the_model_says(st, model, dig)


# ---- after the collect ---------------------------------------------------------------------
def test_the_layer_goes_on_after_a_collect():
    import chunkfs_amd as c
    lengths = [900, 1800, 64, 4000, 250, 1234]
    data = rand(10, sum(lengths))
    p = GcPair(c)
    interleave(p, data, lengths, {0, 3, 4})
    p.remove("dead")
    p.collect()
    # equal to a survivor: not new; equal to a dropped chunk: new
    d_data = sm.dev(data)
    chunks = _tiling(lengths)
    dig, want = p.m.store.put(data, chunks)
    assert want.tolist() == [True, False, False, True, True, False]
    assert sm.put(p.fs.store, d_data, data.size, chunks, dig).tolist() == want.tolist()
    p.check_all()
    p.append(p.file("keep"), data, chunks[[4, 1]])  # append to a survivor
    p.append(p.file("new"), data, [[10, 3000]])
    ch = c.FSChunker(512)
    h2, d2 = p.create("batch", ch), rand(11, 2048)
    keep_w = p.open("keep", ch)
    assert p.fs.write_to_files([keep_w[0], h2[0]], [data[:1024], d2]) == [2, 4]  # over a kept and a new file
    p.m.append_lengths(keep_w[1], data[:1024], [512, 512])
    p.m.append_lengths(h2[1], d2, [512] * 4)
    p.seen.update(p.m.hashes(keep_w[1]) + p.m.hashes(h2[1]))
    p.check_all()
    r = p.collect()  # drops what the bare put above stored for nobody
    assert r["containers_after"] < r["containers_before"]
    p.check_all()
    r = p.collect()  # a second collect is a no-op
    assert r["bytes_moved"] == 0 and r["containers_before"] == r["containers_after"]
    assert r["arena_used_before"] == r["arena_used_after"]
    p.check_all()


def test_collect_then_scrub_then_reads():
    import chunkfs_amd as c
    lengths = [700, 2100, 4096, 33, 1500]
    data = rand(12, sum(lengths))
    fs = c.FileSystem.new_with_scrubber(c.CopyScrubber(), max_chunks=256, arena_bytes=MB,
                                        target_max_chunks=256, target_arena_bytes=MB, seg_size=8192)
    p = GcPair(c, fs=fs)
    interleave(p, data, lengths, {1, 3})
    p.remove("dead")
    r = p.collect()  # a target is attached but nothing is scrubbed yet: allowed
    assert r["containers_after"] == 3
    p.check_all()
    assert fs.scrub().processed_data == 700 + 4096 + 1500
    for name in p.m.list():
        p.check_reads(name)
    # scrubbed now: CDC_ENOTSUP, nothing changed
    before = repr((fs.store.stats(), fs.store.scrub_stats()))
    with pytest.raises(c.CdcError) as e:
        fs.collect()
    assert _code(e) == c._lib.CDC_ENOTSUP
    with pytest.raises(c.CdcError) as e:
        fs.store.retain(_digests(data, _tiling(lengths))[:1])
    assert _code(e) == c._lib.CDC_ENOTSUP
    assert repr((fs.store.stats(), fs.store.scrub_stats())) == before
    for name in p.m.list():
        p.check_reads(name)


def test_collecting_a_target_store_is_the_base_s_target_cleared():
    import chunkfs_amd as c
    data = rand(13, 3000)
    fs = c.FileSystem.new_with_scrubber(c.CopyScrubber(), max_chunks=64, arena_bytes=MB,
                                        target_max_chunks=64, target_arena_bytes=MB)
    h = fs.create_file("x", c.FSChunker(1000))
    fs.write_to_file(h, data)
    fs.scrub()
    assert (fs.read_file_complete(h) == data).all()
    dig = fs.hashes(h)
    assert fs.target.retain(dig[:2]) == 2  # the target itself holds plain chunks: allowed
    with pytest.raises(c.CdcError) as e:
        fs.read_file_complete(h)
    assert _code(e) == c._lib.CDC_ENOTFOUND  # as after cdc_store_clear(target)


# ---- reclaiming space: the reason for the feature -------------------------------------------
def test_a_refused_write_succeeds_after_remove_and_collect():
    import chunkfs_amd as c
    p = GcPair(c, max_chunks=64, arena=40000)
    blocks = [rand(20 + i, 9000) for i in range(5)]
    for i in range(4):
        p.append(p.file(f"f{i}"), blocks[i], [[0, 4000], [4000, 5000]])
    late = p.file("late")
    before = p.fs.store.stats()
    with pytest.raises(c.CdcError) as e:
        Pair.append(p, late, blocks[4], [[0, 4000], [4000, 5000]])  # 4 * 9008 + 9008 > 40 000
    assert _code(e) == c._lib.CDC_ENOMEM and p.fs.store.stats() == before
    p.remove("f1")
    with pytest.raises(c.CdcError) as e:  # remove alone gives nothing back
        Pair.append(p, late, blocks[4], [[0, 4000], [4000, 5000]])
    assert _code(e) == c._lib.CDC_ENOMEM
    r = p.collect()
    assert r["arena_used_before"] - r["arena_used_after"] == 9008
    p.append(late, blocks[4], [[0, 4000], [4000, 5000]])
    p.check_all()


# ---- the C++ mirror ----------------------------------------------------------------------------
def test_cpp_collect_example_runs():
    import subprocess
    from chunkfs_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "_build", "files_collect_example")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(root, "include"), "-isystem", os.path.join(rocm, "include"),
                    os.path.join(root, "examples", "files_collect_example.cpp"),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd", "-L", os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
                    "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "collect ok: 16 containers kept, 65536 bytes moved" in r.stdout and "98304 bytes in use" in r.stdout


# ---- staleness ---------------------------------------------------------------------------------
def test_a_second_layer_and_a_file_from_before_a_clear_are_stale_not_wrong():
    import chunkfs_amd as c
    data = rand(14, 6000)
    p = GcPair(c)
    old = p.file("old")
    p.append(old, data, [[0, 1000]])
    p.fs.store.clear()  # `old` is stale from here on: no root of a collect
    p.m.store.__init__()
    p.seen.clear()
    interleave(p, data, [500, 1500, 2500], {0})
    other = c.FileSystem(store=p.fs.store)  # a second layer on the same store
    oh = other.create_file("theirs", None)
    d_data, ch = sm.dev(data), _tiling([1500, 800])
    dd, dc = sm.dev(_digests(data[500:], ch)), sm.dev_chunks(ch)
    assert other.append_device(oh, d_data.data_ptr() + 500, 2300, dc.data_ptr(), dd.data_ptr(), 2) == 2
    p.m.store.put(data[500:], ch)  # [500, 2000) is `keep`'s too; [2000, 2800) only the other layer's
    p.seen.update(bytes(d) for d in _digests(data[500:], ch))
    assert (other.read_file_complete(oh) == data[500:2800]).all()
    p.remove("dead")
    p.m.remove("old")  # the model has no epochs: a stale file references nothing
    r = p.collect()
    assert r["containers_after"] == 2  # the other layer's own chunk is gone
    p.check_store()
    p.check_reads("keep")
    for stale in (old[0], ):
        for call in (lambda: p.fs.read_file_complete(stale), lambda: p.fs.pread(stale, 0, 10)):
            with pytest.raises(c.CdcError) as e:
                call()
            assert _code(e) == c._lib.CDC_ENOTFOUND
    with pytest.raises(c.CdcError) as e:
        other.read_file_complete(oh)
    assert _code(e) == c._lib.CDC_ENOTFOUND
    assert p.fs.stat(old[0])["size"] == 1000  # still there, still stale
