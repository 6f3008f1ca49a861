"""The power of the call sequences of tests/history_harness.py, with the CPU
oracle alone (no GPU): a result computed from the state an earlier call left
behind must be visibly different from the right one, or tests/test_gpu_history.py
could pass over it.  These are conditions on the inputs -- seeds and lengths
were picked until they hold for every call; none is exempt."""
import json
import os

import numpy as np
import pytest

import history_harness as hh
import oracle

@pytest.mark.parametrize("name", hh.NAMES)
def test_stale_answers_are_visible(name):
    """For every call: its answer differs from the answer of the call 1, 3 and
    4 back (the previous call, the host staging block's last user, the device
    slot's / ring slot's), and from its own bytes cut with that call's
    lengths."""
    assert hh.get(name).name == name and hh.power_violations(hh.get(name)) == []


def test_s1_stale_entry_and_stale_length_differ():
    """S1: "the host read h_out_ too early" (the earlier call's list) and "the
    device used an old length" (this buffer cut at the earlier length) give
    different (offset, length) pairs for the calls 1 and 3 back, which used
    the other base buffer.  Two cases cannot differ whatever the bytes, and
    are checked to be exactly those: a list of one chunk (0, n) -- an earlier
    length no longer than both buffers' first cuts --, and the call 4 back,
    which used the same buffer (its list IS this buffer cut at its length)."""
    seq = hh.s1()
    calls = hh.model(seq)
    fa, fb = (int(oracle.fastcdc(seq.buffers[b], *seq.sizes)[0, 1]) for b in "AB")
    assert fa != fb
    told_apart = 0
    for ci in range(2 + 4, len(calls)):  # the sweep (after the two big calls)
        c = calls[ci]
        for d in hh.DISTANCES:
            j = calls[ci - d]
            alt = c.with_lengths_of(j)
            assert alt is not None  # (no length repeats)
            if d == 4:
                assert j.streams[0][0] == c.streams[0][0] and hh.same_lists(alt, j.ref.lists)
            elif j.streams[0][2] <= min(fa, fb):
                assert hh.same_lists(alt, j.ref.lists) and len(alt[0]) <= 1
            else:
                assert j.streams[0][0] != c.streams[0][0] and not hh.same_lists(alt, j.ref.lists), (c.index, d)
                told_apart += 1
    assert told_apart > 800


def test_s1_is_the_recorded_state():
    seq = hh.s1()
    assert [op[1][0][2] for op in seq.ops[:2]] == [3 * (1 << 20) + 17, 1 << 20]
    lens = [op[1][0][2] for op in seq.ops[2:]]
    assert sorted(lens) == sorted(hh.tails_lengths()) and lens != sorted(lens)
    assert [op[1][0][0] for op in seq.ops[2:6]] == ["A", "B", "A", "B"]
    assert {8146, 16390} <= set(lens)  # the two lengths of the red runs


def test_s2_slots_golden_and_stale_blocks():
    seq = hh.s2()
    calls = hh.model(seq)
    n = [c.streams[0][2] for c in calls]
    assert len(calls) >= 9 and all(x <= 4 << 20 for x in n)  # one ring slot per call
    assert min(sum(1 for i in range(len(n)) if i % hh.RING_SLOTS == s) for s in range(hh.RING_SLOTS)) >= 3
    # a slot's earlier, longer content lies beyond the new length
    beyond = [i for i in range(len(n)) if any(n[j] > n[i] for j in range(i % hh.RING_SLOTS, i, hh.RING_SLOTS))]
    assert len(beyond) >= 6 and hh.S2_GOLDEN_AT in beyond
    # the golden vector, after other content in its slot and in the call before
    g = calls[hh.S2_GOLDEN_AT]
    with open(os.path.join(os.path.dirname(__file__), "golden", "fastcdc_selfconsistent.json")) as f:
        vec = [v for v in json.load(f)["vectors"] if (v["pattern"], v["len"], v["seed"]) == hh.GOLDEN][0]
    assert (vec["min"], vec["avg"], vec["max"]) == seq.sizes
    assert [int(x) for x in g.ref.lists[0][:, 1]] == vec["lengths"]
    assert n[hh.S2_GOLDEN_AT - hh.RING_SLOTS] >= 1 << 20 and n[hh.S2_GOLDEN_AT - 1] >= 1 << 20
    # stale bytes in any 32 KiB block would move a cut: the device copy
    # (rewritten by every call) and the ring slot (by every fourth)
    for every, at_least in ((1, 400), (hh.RING_SLOTS, 100)):
        bad, blocks = hh.stale_block_violations(seq, every)
        assert bad == [] and blocks >= at_least


def test_s3_visits_every_regime_and_reuses_the_slots():
    seq = hh.s3()
    calls = hh.model(seq)
    kinds = {"small": 0, "zero_copy": 0, "uploaded": 0, "pipeline": 0, "empty": 0, "none": 0}
    submits, at = [], {}
    for c in calls:
        n, total = len(c.streams), sum(s[2] for s in c.streams)
        light = c.index in seq.light
        if n == 0:
            kinds["none"] += 1
        elif total == 0:
            kinds["empty"] += 1
        elif n == 1 and total <= 4 << 20:
            kinds["small"] += 1
        elif total <= 8 << 20 and n <= 64:
            kinds["zero_copy"] += 1
        elif total <= 8 << 20:
            kinds["uploaded"] += 1
        else:
            kinds["pipeline"] += 1
        assert light == (n == 0 or (n == 1 and 0 < total <= 4 << 20))  # what goes through no submit
        if not light:
            at[c.index] = len(submits)
            submits.append(c)
    assert all(v >= 2 for v in kinds.values()), kinds
    # same pointers four submits later (the same device slot): every length + 1,
    # then the same lengths with rewritten bytes
    for a, b, c2 in ((2, 7, 18), (4, 9, 20)):
        A, B, C = (calls[[c.index for c in calls].index(i)] for i in (a, b, c2))
        assert at[b] - at[a] == 4 and at[c2] - at[b] == 4
        assert [(s[0], s[1], s[2] + 1) for s in A.streams] == list(B.streams) and B.streams == C.streams
        assert not hh.same_lists(B.ref.lists, C.ref.lists)
    big, one = calls[[c.index for c in calls].index(23)], calls[[c.index for c in calls].index(24)]
    assert sum(s[2] for s in big.streams) >= (40 << 20) - 1024 and at[24] == at[23] + 1
    assert sum(s[2] for s in one.streams) <= 16384 and len(one.streams) > 1  # one span, not the small kernel


def test_s4_burst_shape():
    seq = hh.s4()
    bursts, cur = [], []
    for op in seq.ops:
        if op[0] == "async":
            cur.append(op[1])
        elif cur:
            bursts.append((cur, op[0]))
            cur = []
    assert [len(b) for b, _ in bursts] == [10, 9] and [e for _, e in bursts] == ["sync", "host"]
    every = [b for burst, _ in bursts for b in burst]
    for k, b in enumerate(every):
        assert sum(s[2] for s in b) > 8 << 20
        if k >= 3:
            assert len(b) != len(every[k - 3])
        if k >= 4:
            p = every[k - 4]
            assert [s[:2] for s in b] == [s[:2] for s in p]
            assert sorted(x[2] - y[2] for x, y in zip(b, p)) == [0] * (len(b) - 1) + [1]


@pytest.mark.parametrize("algo", hh.WALK_ALGOS)
def test_s5_shape(algo):
    seq = hh.s5(algo)
    calls = hh.model(seq)
    zc, m65, big = calls[0], calls[1], calls[2]
    assert len(zc.streams) <= 64 and sum(s[2] for s in zc.streams) <= 8 << 20
    assert len(m65.streams) == 65 and sum(s[2] for s in big.streams) > 8 << 20
    asyncs = [c for c in calls if c.kind == "async"]
    assert len(asyncs) == 4 and all(sum(s[2] for s in c.streams) > 8 << 20 for c in asyncs)
    again = calls[5]
    assert [(s[0], s[1], s[2] + 1) for s in zc.streams] == list(again.streams)
    quiet = calls[6]
    assert (quiet.arrays[0][700001:1300001] == 0).all()
    if algo == "rabin":  # the polynomial matters for every result after it
        for c in calls[5:]:
            assert c.rabin_poly == hh.SECOND_POLY
            old = [oracle.cdc("rabin", c.arrays[k][o:o + n], *seq.sizes) for k, (_, o, n) in enumerate(c.streams)]
            assert not hh.same_lists(old, c.ref.lists)


def test_s6_the_table_matters_on_every_path():
    calls = hh.model(hh.s6())
    half = len(calls) // 2
    assert [c.kind for c in calls[:half]] == [c.kind for c in calls[half:]]
    assert {c.kind for c in calls} == {"host", "batch", "async", "write"}
    for before, after in zip(calls[:half], calls[half:]):
        assert before.streams == after.streams and before.table is None and after.table is not None
        assert not hh.same_lists(before.ref.lists, after.ref.lists)  # a stale table gives `before`


def test_s7_first_write_carries_a_chunk():
    seq = hh.s7()
    w1, h, w2 = hh.model(seq)
    # the first write fills a 256 MiB device window: that window's last chunk
    # (never empty) is carried into the other window, and stays there
    assert w1.streams[0][2] > (256 << 20) > w2.streams[0][2] and h.kind == "host"
    assert not np.array_equal(w1.arrays[0][:w2.streams[0][2]], w2.arrays[0][:w2.streams[0][2]])


def test_mismatch_message_names_the_stale_call():
    """The harness diagnoses itself: handed the answer a stale state would
    give, the message names the op, the history and the earlier call."""
    seq = hh.s1()
    calls = hh.model(seq)
    ci = 400
    c, prev = calls[ci], calls[ci - 1]
    assert hh.diagnose(seq, ci, hh.Result(c.ref.lists)) is None
    msg = hh.diagnose(seq, ci, hh.Result(prev.ref.lists))
    assert f"op {c.index} " in msg and f"WHOLE answer of op {prev.index} " in msg and "history" in msg
    assert f"{prev.index} host(" in msg
    msg = hh.diagnose(seq, ci, hh.Result(c.with_lengths_of(calls[ci - 3])))
    assert f"cut with op {calls[ci - 3].index}'s length" in msg and "3 calls back" in msg
    # the last entry alone stale, as in the red runs ([6060, 2085] for [6060, 2086])
    k = next(i for i in range(10, len(calls)) if calls[i].streams[0][0] == calls[i - 4].streams[0][0]
             and len(calls[i].ref.lists[0]) == len(calls[i - 4].ref.lists[0]) >= 2)
    got = calls[k].ref.lists[0].copy()
    got[-1] = calls[k - 4].ref.lists[0][-1]
    msg = hh.diagnose(seq, k, hh.Result([got]))
    assert f"op {calls[k - 4].index}'s list entry" in msg
