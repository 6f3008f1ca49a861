"""The AE model itself (tests/ae_model.py, no GPU): the numpy form against the
literal byte-serial rule, known answers worked out by hand, and the statistics
that show the parity tests exercise the content rule and not the max clamp."""
import numpy as np
import pytest

import ae_model as ae

PARAMS = [(16, 64, 256, 1), (100, 200, 400, 63), (8, 128, 300, 64), (8, 128, 300, 65), (64, 256, 1024, 149),
          (512, 1024, 4096, 595)]


def _inputs():
    rng = np.random.default_rng(7)
    n = 50000
    return {
        "random": rng.integers(0, 256, n, dtype=np.uint8),
        "random300k": rng.integers(0, 256, 300000, dtype=np.uint8),
        "3symbol": rng.integers(0, 3, n, dtype=np.uint8),
        "constant": np.full(n, 0x5A, dtype=np.uint8),
        "ascending": (np.arange(n) % 256).astype(np.uint8),
        "descending": (255 - np.arange(n) % 256).astype(np.uint8),
    }


INPUTS = _inputs()


def _tiles(ch, n, mn, mx):
    at = 0
    for i, (o, ln) in enumerate(ch):
        assert o == at and 0 < ln <= mx
        assert ln >= mn or i == len(ch) - 1
        at += ln
    assert at == n


@pytest.mark.parametrize("name", sorted(INPUTS))
@pytest.mark.parametrize("mode", [ae.MAX, ae.MIN])
def test_numpy_form_equals_the_literal_rule(name, mode):
    data = INPUTS[name]
    sets = PARAMS if name != "random300k" else [PARAMS[0], PARAMS[-1]]
    for mn, avg, mx, w in sets:
        lit = ae.chunks(data, mn, avg, mx, w, mode, fast=False)
        fast = ae.chunks(data, mn, avg, mx, w, mode)
        assert lit == fast, (name, mode, mn, avg, mx, w)
        _tiles(lit, len(data), mn, mx)


@pytest.mark.parametrize("mode", [ae.MAX, ae.MIN])
@pytest.mark.parametrize("byte", [0x00, 0xAA, 0xFF])
def test_constant_data_cuts_at_max_of_min_and_window_plus_one(mode, byte):
    # no value is ever better than M's, so the cut comes `window` past s + skip
    data = np.full(20000, byte, dtype=np.uint8)
    for mn, avg, mx, w in PARAMS:
        ch = ae.chunks(data, mn, avg, mx, w, mode, fast=False)
        assert {ln for _, ln in ch[:-1]} == {max(mn, w + 1)}
        assert ch == ae.chunks(data, mn, avg, mx, w, mode)


def test_strictly_ascending_values_never_cut_early():
    # bytes 0..255: v(i) rises with its leading byte, the padded tail included
    data = np.arange(256, dtype=np.uint8)
    v = [ae.value(data, i) for i in range(256)]
    assert all(a < b for a, b in zip(v, v[1:]))
    for fast in (False, True):
        assert ae.chunks(data, 8, 16, 32, 4, ae.MAX, fast=fast) == [(o, 32) for o in range(0, 256, 32)]
        assert ae.chunks(data[::-1].copy(), 8, 16, 32, 4, ae.MIN, fast=fast) == [(o, 32) for o in range(0, 256, 32)]
    # ... and the other mode cuts as early as it may: every value is worse than M's
    assert {ln for _, ln in ae.chunks(data, 8, 16, 32, 4, ae.MIN)[:-1]} == {8}


def test_value_pads_with_zeros_at_the_buffer_end():
    data = np.array([1, 2, 3, 4, 5], dtype=np.uint8)
    assert ae.value(data, 0) == 0x01020304 and ae.value(data, 1) == 0x02030405
    assert ae.value(data, 2) == 0x03040500 and ae.value(data, 4) == 0x05000000
    assert list(ae.values(data, ae.MAX)) == [ae.value(data, i) for i in range(5)]
    assert list(ae.values(data, ae.MIN)) == [0xFFFFFFFF - ae.value(data, i) for i in range(5)]


def test_default_window():
    assert ae.default_window(8192) == 4767
    assert ae.default_window(1) == 1
    assert ae.default_window(0xFFFFFFFF) == 0xFFFFFFFF * 100000 // 171828


@pytest.mark.parametrize("sizes", [(64, 256, 1024), (512, 1024, 4096)])
def test_mean_length_and_max_forced_share_at_the_default_window(sizes):
    mn, avg, mx = sizes
    data = INPUTS["random300k"]
    ln = np.array([x for _, x in ae.chunks(data, mn, avg, mx)][:-1])
    mean, forced = ln.mean(), (ln == mx).mean()
    print(f"AE {sizes} window {ae.default_window(avg)}: mean {mean:.1f}, max-forced {forced:.4f}")
    assert 0.9 * avg <= mean <= 1.2 * avg
    assert forced < 0.05


def test_storage_writer_loop():
    data = np.random.default_rng(3).integers(0, 256, (2 << 20) + 4321, dtype=np.uint8)
    spans = ae.storage_writer(data, 512, 1024, 4096)
    assert sum(spans) == len(data) and all(0 < x <= 4096 for x in spans)
    # one segment: the loop is one chunk_data
    one = data[:300000]
    assert ae.storage_writer(one, 512, 1024, 4096) == [x for _, x in ae.chunks(one, 512, 1024, 4096)]
    # a cut that lands in the last bytes of a segment's buffer reads the zero
    # padding: the loop is the rule per buffer, and need not equal one
    # chunk_data over the whole write
    seg = 1000
    one = (one % 3).astype(np.uint8)  # (values tie in their leading bytes: the padding decides)
    spans2 = ae.storage_writer(one, 16, 64, 256, 1, seg=seg)
    assert sum(spans2) == len(one)
    assert spans2 != [x for _, x in ae.chunks(one, 16, 64, 256, 1)]
    rest, ref = np.empty(0, dtype=np.uint8), []
    for off in range(0, len(one), seg):
        buf = np.concatenate([rest, one[off:off + seg]])
        ch = ae.chunks(buf, 16, 64, 256, 1, fast=False)
        ref += [x for _, x in ch[:-1]]
        rest = buf[ch[-1][0]:]
    assert spans2 == ref + [len(rest)]
