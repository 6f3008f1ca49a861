"""The BLAKE2sp model (tests/blake2sp_model.py) against hashlib: the twin that is
written the way blake2sp.hip is equals the oracle at every length where the
kernel takes another path, the three known answers are pinned, and the
compression carries a byte counter past 2^32."""
import os

import numpy as np

import blake2sp_model as bm


def test_known_answers():
    for data, want in bm.KNOWN.items():
        assert bm.oracle(data).hex() == want
        assert bm.blake2sp(data).hex() == want
    assert len(bm.KNOWN) == 3


def test_twin_equals_hashlib_for_every_length_to_1100():
    rng = np.random.default_rng(11)
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in range(1101)]
    got = bm.blake2sp_many(datas)
    bad = [n for n, (g, d) in enumerate(zip(got, datas)) if g != bm.oracle(d)]
    assert not bad, bad[:20]


def test_twin_equals_hashlib_at_4096_and_16384():
    datas = [os.urandom(n) for n in (4096, 16384)] + [bytes(4096), bytes(16384)]
    assert bm.blake2sp_many(datas) == [bm.oracle(d) for d in datas]


def test_twin_equals_hashlib_at_16_mib():
    data = np.random.default_rng(12).integers(0, 256, 16 << 20, dtype=np.uint8).tobytes()
    assert bm.blake2sp(data) == bm.oracle(data)


def test_groups_of_unequal_length_step_together():
    """A long chunk beside short ones: the groups leave at different steps."""
    datas = [os.urandom(n) for n in (70000, 0, 1, 513, 64, 4097, 511, 512)]
    assert bm.blake2sp_many(datas) == [bm.oracle(d) for d in datas]


def test_param_words_are_the_parameter_block():
    """IV ^ the 32-byte parameter block, as RFC 7693 2.5 lays it out."""
    for off, root in ((0, False), (7, False), (0, True), ((1 << 40) + 5, False)):
        block = bytes([32, 0, 8, 2]) + (0).to_bytes(4, "little") + off.to_bytes(6, "little") + \
            bytes([1 if root else 0, 32]) + bytes(16)
        words = np.frombuffer(block, dtype="<u4")
        assert bm.param_words(off, root) == [int(i) ^ int(w) for i, w in zip(bm.IV, words)]


def test_compress_carries_a_counter_past_2_to_32():
    """A leaf longer than 4 GiB: no such buffer here, so the counter is
    synthetic.  The vector compression and the integer one agree for counters on
    both sides of 2^32, the high word reaches v[13] (a counter that differs only
    there gives another state), and hashlib confirms the low side."""
    rng = np.random.default_rng(13)
    m = [int(x) for x in rng.integers(0, 1 << 32, 16, dtype=np.uint64)]
    h = bm.param_words(3, False)
    ts = [64, (1 << 32) - 64, 1 << 32, (1 << 32) + 64, (5 << 32) + 128, (1 << 63) + 64]
    ha = np.repeat(np.array(h, dtype=np.uint32)[:, None], len(ts), axis=1)
    ma = np.repeat(np.array(m, dtype=np.uint32)[:, None], len(ts), axis=1)
    zero = np.zeros(len(ts), dtype=np.uint32)
    got = bm.compress(ha, ma, np.array(ts, dtype=np.uint64), zero, zero)
    outs = []
    for i, t in enumerate(ts):
        want = bm.compress_int(h, m, t, 0, 0)
        assert [int(x) for x in got[:, i]] == want, hex(t)
        outs.append(tuple(want))
    assert len(set(outs)) == len(ts)
    assert outs[0] != tuple(bm.compress_int(h, m, 64 + (1 << 32), 0, 0))
    # the low side against hashlib: one final 64-byte block of leaf 3
    import hashlib
    block = np.array(m, dtype="<u4").tobytes()
    ref = hashlib.blake2s(block, digest_size=32, fanout=8, depth=2, leaf_size=0, inner_size=32, node_offset=3,
                          node_depth=0, last_node=False).digest()
    assert np.array(bm.compress_int(h, m, 64, bm.M32, 0), dtype="<u4").tobytes() == ref
