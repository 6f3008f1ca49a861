"""CPU suite of removal and collection: the model of tests/gc_model.py against a
twin that only ever saw the surviving files, and the move planner against the
safety rule it must keep.  No device, no library call."""
import random

import numpy as np
import pytest

import files_model as fm
import gc_model as gm
import store_model as sm


def blob(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def tile(lengths):
    lengths = np.asarray(lengths, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64)
    return np.stack([offs, lengths], axis=1)


def replay(log, keep):
    """A twin layer that was only handed the writes of the files in `keep`."""
    twin, handles = gm.Files(seg_size=6000), {}
    for name, data, chunks in log:
        if name in keep:
            if name not in handles:
                handles[name] = twin.create(name)
            twin.append(handles[name], data, chunks)
    for name in keep:
        if name not in handles:
            handles[name] = twin.create(name)
    return twin


def assert_equals_twin(fs, twin):
    assert fs.store.stats() == twin.store.stats()
    assert set(fs.store.db) == set(twin.store.db)
    assert fs.list() == twin.list()
    for name in fs.list():
        a, b = fs.open(name), twin.open(name)
        assert (fs.read_complete(a) == twin.read_complete(b)).all()
        assert fs.hashes(a) == twin.hashes(b)
        assert fs.distribution(a) == twin.distribution(b)
        size = fs.size(a)
        for off, ln in [(0, size), (size // 3, size // 2), (max(size - 5, 0), 9)]:
            assert (fs.pread(a, off, ln) == twin.pread(b, off, ln)).all()
        while True:
            x, y = fs.read(a), twin.read(b)
            assert (x == y).all()
            if not len(x):
                break


def random_layer(seed, files=6, writes=14):
    rnd = random.Random(seed)
    pool = [blob(seed * 100 + i, rnd.choice([0, 1, 15, 16, 17, 300, 4095, 4096, 4097])) for i in range(12)]
    fs, log, handles = gm.Files(seg_size=6000), [], {}
    for _ in range(writes):
        name = f"f{rnd.randrange(files)}"
        if name not in handles:
            handles[name] = fs.create(name)
        parts = [pool[rnd.randrange(len(pool))] for _ in range(rnd.randrange(1, 6))]
        data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        chunks = tile([len(p) for p in parts])
        fs.append(handles[name], data, chunks)
        log.append((name, data, chunks))
    return fs, log, rnd


@pytest.mark.parametrize("seed", range(8))
def test_collect_equals_a_twin_that_wrote_only_the_survivors(seed):
    fs, log, rnd = random_layer(seed)
    names = fs.list()
    gone = set(rnd.sample(names, len(names) // 2))
    for name in gone:
        fs.remove(name)
    dropped = set(fs.store.db) - set(fs.refs())
    order_before = [k for k in fs.store.db if k not in dropped]
    r = fs.collect()
    assert_equals_twin(fs, replay(log, set(names) - gone))
    assert list(fs.store.db) == order_before, "the survivors keep their relative arena order"
    assert r["containers_after"] == len(order_before) and r["arena_used_after"] == fs.store.stats()["arena_used"]
    assert all(not fs.store.contains(k) for k in dropped)
    # idempotence: a second collect drops nothing, moves nothing and leaves the same layer
    before = (fs.store.stats(), dict(fs.store.db))
    r2 = fs.collect()
    assert (fs.store.stats(), dict(fs.store.db)) == before
    assert r2["bytes_moved"] == 0 and r2["groups_direct"] == r2["groups_bounced"] == 0
    assert r2["containers_before"] == r2["containers_after"]


def test_a_digest_shared_by_a_removed_and_a_kept_file_survives_and_a_dead_one_comes_back_as_new():
    shared, only_a, only_b = blob(1, 500), blob(2, 700), blob(3, 900)
    fs = gm.Files()
    a, b = fs.create("a"), fs.create("b")
    fs.append(a, np.concatenate([only_a, shared]), tile([700, 500]))
    fs.append(b, np.concatenate([shared, only_b]), tile([500, 900]))
    fs.remove("a")
    with pytest.raises(fm.ModelError) as e:
        fs.read_complete(a)  # the handle holds the name
    assert e.value.code == fm.ENOTFOUND
    r = fs.collect()
    assert (r["containers_before"], r["containers_after"]) == (3, 2)
    assert fs.store.contains(fm.sha(shared)) and fs.store.contains(fm.sha(only_b))
    assert not fs.store.contains(fm.sha(only_a))
    assert fs.store.stats() == {"chunks_written": 2, "bytes_written": 1400, "unique_chunks": 2, "unique_bytes": 1400,
                                "arena_used": 512 + 912}
    assert (fs.read_complete(b) == np.concatenate([shared, only_b])).all()
    # the dropped chunk is new again, the surviving one is not; the new one goes to the end of the arena
    _, new = fs.store.put(np.concatenate([only_a, shared]), tile([700, 500]))
    assert new.tolist() == [True, False]
    assert list(fs.store.locs().values()) == [0, 512, 512 + 912]
    # a file of the removed name is a new, empty file
    a2 = fs.create("a")
    assert fs.size(a2) == 0 and fs.size(a) == 0


def test_remove_of_an_unknown_name_and_retain_of_an_unknown_digest_change_nothing():
    fs = gm.Files()
    h = fs.create("x")
    fs.append(h, blob(5, 100), tile([60, 40]))
    before = (fs.store.stats(), dict(fs.store.db), fs.list())
    with pytest.raises(fm.ModelError) as e:
        fs.remove("y")
    assert e.value.code == fm.ENOTFOUND
    with pytest.raises(fm.ModelError) as e:
        fs.store.retain([fm.sha(blob(5, 100)[:60]), fm.sha(b"absent")])
    assert e.value.code == fm.ENOTFOUND
    assert (fs.store.stats(), dict(fs.store.db), fs.list()) == before


def test_retain_counts_duplicates_as_references_and_zero_digests_keep_nothing():
    st = gm.Store()
    data = blob(7, 1000)
    dig, _ = st.put(data, tile([100, 200, 300, 400]))
    assert st.retain([dig[3], dig[1], dig[3]]) == 2
    assert st.stats() == {"chunks_written": 3, "bytes_written": 1000, "unique_chunks": 2, "unique_bytes": 600,
                          "arena_used": 208 + 400}
    assert list(st.db) == [bytes(dig[1]), bytes(dig[3])]  # arena order, not request order
    assert st.retain([]) == 0
    assert st.stats() == {"chunks_written": 0, "bytes_written": 0, "unique_chunks": 0, "unique_bytes": 0,
                          "arena_used": 0}


# ---- the move planner -------------------------------------------------------------
def layout(lengths, dead):
    """(locs, pads) of the survivors of containers of `lengths` laid back to back."""
    locs, pads, at = [], [], 0
    for i, n in enumerate(lengths):
        if i not in dead:
            locs.append(at)
            pads.append(sm.round_up16(n))
        at += sm.round_up16(n)
    return locs, pads


def test_nothing_dead_or_only_the_tail_dead_moves_nothing():
    assert gm.plan_groups(*layout([100, 200, 300], set())) == []
    assert gm.plan_groups(*layout([100, 200, 300], {2})) == []
    assert gm.plan_groups([], []) == []


def test_a_small_gap_bounces_until_the_gap_has_grown():
    # 16 dead bytes in front of 8 x 4096: every survivor overlaps its own destination
    locs, pads = layout([16] + [4096] * 8, {0})
    g = gm.plan_groups(locs, pads, w_req=8192)
    assert g == [(0, 2, 8192, False), (2, 4, 8192, False), (4, 6, 8192, False), (6, 8, 8192, False)]
    # one container of bounce: a group per container
    assert len(gm.plan_groups(locs, pads, w_req=1)) == 8
    # the default W is the bytes to move: a single bounced group
    assert gm.plan_groups(locs, pads) == [(0, 8, 8 * 4096, False)]


def test_groups_turn_direct_once_the_gap_reaches_half_a_bounce():
    # every second container dead: the gap grows by 4096 per survivor
    lengths = [4096] * 32
    locs, pads = layout(lengths, set(range(0, 32, 2)))
    g = gm.plan_groups(locs, pads, w_req=4 * 4096)
    kinds = [d for *_, d in g]
    assert kinds[0] is False and kinds[-1] is True
    assert kinds == sorted(kinds), "bounced groups first, direct groups once the gap allows"
    gm.check_groups_are_safe(locs, pads, g, 4 * 4096)
    # a large dead prefix: everything slides in one direct group
    locs, pads = layout([1 << 20] + [4096] * 16, {0})
    assert gm.plan_groups(locs, pads) == [(0, 16, 16 * 4096, True)]


def test_length_zero_containers_ride_along():
    locs, pads = layout([0, 100, 0, 50, 0, 4097, 0], {1})
    g = gm.plan_groups(locs, pads, w_req=64)
    gm.check_groups_are_safe(locs, pads, g, 64)
    assert g[0][0] == 1, "the length-0 container in front of the dead one has gap 0 and stays"
    assert sum(x[2] for x in g) == 64 + 4112


@pytest.mark.parametrize("seed", range(40))
def test_random_plans_are_safe_and_cover_every_moved_survivor_once(seed):
    rnd = random.Random(seed)
    lengths = [rnd.choice([0, 1, 15, 16, 17, 100, 4095, 4096, 4097, 20000]) for _ in range(rnd.randrange(1, 60))]
    dead = {i for i in range(len(lengths)) if rnd.random() < rnd.choice([0.1, 0.5, 0.9])}
    locs, pads = layout(lengths, dead)
    w = rnd.choice([1, 4096, 4112, 65536, gm.DEFAULT_BOUNCE])
    g = gm.plan_groups(locs, pads, w)
    gm.check_groups_are_safe(locs, pads, g, w)
    if g:
        assert all(x[1] == y[0] for x, y in zip(g, g[1:])) and g[-1][1] == len(locs)
        newloc = np.concatenate([[0], np.cumsum(pads)])
        assert all(locs[i] == newloc[i] for i in range(g[0][0])), "what is not in a group is in place already"
    else:
        assert locs == list(np.concatenate([[0], np.cumsum(pads)])[:-1]) or not locs
