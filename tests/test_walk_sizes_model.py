"""CPU guard of the walk chunkers' size table (tests/walk_sizes.py): the table
reaches every segment size, both walk modes and both ends of the LeapCDC
threshold table; each small-segment case has an input whose chunks run over
many segments; the model's workspace stays small; validate()'s refusals are
pinned (they are made before any device call).

What the GPU suite then runs over the table is test_gpu_walk_sizes.py."""
import numpy as np
import pytest

import oracle
import walk_sizes as ws

MIB = ws.MIB

ALL = [(c, ws.params(c.algo, *ws.sizes_of(c), cfg=c.cfg)) for c in ws.CASES]


def test_table_is_valid_and_unique():
    seen = set()
    for c, p in ALL:
        assert c.algo in ws.ALGOS and 0 < c.min <= c.avg <= c.max <= ws.U32, c
        assert c.n <= ws.N_MAX and (c.max != ws.U32 or c.n == ws.N_TOP), c
        assert c.n == min(3 * c.max + c.min + 12345, ws.N_MAX) or c.max == ws.U32, c
        key = (c.algo, c.min, c.avg, c.max, c.cfg)
        assert key not in seen, c
        seen.add(key)
        assert (c.pattern is not None) == (c.group == "small" and c.max >= 4 << p.seg_log2), c
        a, b = ws.zero_region(c)
        assert a & 1 and 0 < a < b < c.n, c
        if c.max + c.max // 2 + 7 <= (c.n - a) // 2:
            assert b - a > c.max, c                       # longer than max where that fits
    for algo in ws.ALGOS:
        for sizes in [(3000, 3000, 3000), (2000, 3000, 3000), (4097, 8191, 16385), (5000, 5001, 5002)]:
            assert any(c.algo == algo and ws.sizes_of(c) == sizes for c in ws.CASES), (algo, sizes)
        assert sum(c.algo == algo for c in ws.SCHEDULE_CASES) == 2, algo
        assert {c.group for c in ws.SCHEDULE_CASES if c.algo == algo} == {"small", "cap"}, algo
    assert len(ws.WRITE_CASES) == 2 and all(c.max == 16 << 20 for c in ws.WRITE_CASES)


def test_model_known_rows():
    """Rows worked out by hand from walk_engine.cpp."""
    p = ws.params("rabin", 4096, 8192, 16384)      # bitmap; 8 avg = 2^16 < 2^17; floor(log2 min) + 12 = 24
    assert (p.nbm, p.warm_mult, p.seg_log2, p.warm, p.cap, p.piece_log2, p.rabin_mask) == \
        (1, 8, 17, 65536, 34, 15, 8191)
    p = ws.params("rabin", 16, 64, 256)            # min < 48: byte mode, 32 KiB; 4 + 12 = 16 does not lower it
    assert (p.nbm, p.mode, p.warm_mult, p.seg_log2, p.cap) == (0, "byte", 8, 15, 2050)
    p = ws.params("seq", 1, 4096, 1048576)         # 0 + 12 = 12; one start per byte and two
    assert (p.nbm, p.seg_log2, p.warm, p.cap, p.piece_log2, p.seg_words) == (1, 12, 65536, 4098, 12, 64)
    p = ws.params("leap", 32768, 262144, 4194304)  # 24 avg = 6 MiB: 2^23, capped at 22
    assert (p.nbm, p.seg_log2, p.warm, p.cap, p.leap_index) == (2, 22, 6291456, 130, 18)
    p = ws.params("leap", 32, ws.U32, ws.U32)      # avg - min = 2^32 - 33 rounds to 2^32; 5 + 12 = 17
    assert (p.seg_log2, p.warm, p.leap_index, p.rabin_mask) == (17, 24 * ws.U32, 32, (1 << 32) - 1)
    assert p.warm > 1 << 36
    p = ws.params("ultra", 8, 8, 8)
    assert (p.nbm, p.seg_log2, p.cap, p.leap_index) == (3, 15, 4098, 0)
    p = ws.params("seq", 300, 1000, 5000, cfg=(0, 64, 5, 10))
    assert (p.nbm, p.warm_mult, p.seg_log2) == (0, 16, 15)
    p = ws.params("seq", 4096, 8192, 16384, walk_bytes=True)
    assert (p.nbm, p.seg_log2) == (0, 15)
    p = ws.params("ae", 4096, 8192, 16384, walk_bytes=True)   # AE has no byte walk
    assert (p.nbm, p.seg_log2, p.window) == (1, 18, 4767)
    p = ws.params("ae", 64, 256, 1024, walk=(10, 2))          # its bitmap pass steps 4 KiB at a time
    assert (p.seg_log2, p.warm) == (12, 512)
    # either side of 2^12.5 = 5792.6
    assert ws.params("rabin", 64, 5792, 20001).rabin_mask == 4095
    assert ws.params("rabin", 64, 5793, 20001).rabin_mask == 8191
    assert ws.params("leap", 64, 64 + 5792, 20001).leap_index == 12
    assert ws.params("leap", 64, 64 + 5793, 20001).leap_index == 13
    assert ws.params("leap", 64, 64, 20001).leap_index == 0
    thr = oracle._cdc_params()["THR"]
    assert len(thr) == 33 and ws.params("leap", 32, ws.U32, ws.U32).leap_thr == thr[32]


def test_model_refuses_what_validate_refuses():
    for algo, sizes, cfg in [("seq", (0, 10, 20), None), ("seq", (100, 50, 200), None), ("seq", (10, 300, 200), None),
                             ("ultra", (7, 8, 16), None), ("leap", (31, 64, 128), None), ("rabin", (1, 1, 2), None),
                             ("ae", (16, 64, 256), 256)]:
        with pytest.raises(ValueError):
            ws.params(algo, *sizes, cfg=cfg)
    ws.params("ae", 16, 64, 256, cfg=255)
    ws.params("rabin", 1, 2, 2)


def test_coverage_of_the_parameter_range():
    assert {p.seg_log2 for _, p in ALL} == set(range(12, 23))
    for algo in ("rabin", "seq"):
        assert {p.mode for c, p in ALL if c.algo == algo} == {"byte", "bitmap"}, algo
    assert {0, 32} <= {p.leap_index for c, p in ALL if c.algo == "leap"}
    assert {p.seg_log2 for c, p in ALL if c.group == "small"} <= set(range(12, 18))
    assert {p.seg_log2 for c, p in ALL if c.group == "cap"} == {22}
    for c, p in ALL:
        if c.group == "cap":
            # the warm-up is a segment or more (avg 256 KiB: 1 and 1.5; avg 1 MiB
            # and up: 4 to 8), so a walk starts in an earlier segment or at the
            # stream start
            assert p.warm >= 1 << p.seg_log2, c
            assert c.avg < MIB or p.warm >= 4 << p.seg_log2, c
        if c.group == "top":
            assert c.max == ws.U32
    assert any(c.avg == ws.U32 and p.rabin_mask == ws.U32 for c, p in ALL if c.algo == "rabin")
    assert any(c.max % 64 for c, _ in ALL) and any(c.min == c.avg == c.max for c, _ in ALL)
    assert {c.algo for c, _ in ALL if c.group == "cap"} == set(ws.ALGOS)
    assert {c.algo for c, _ in ALL if c.group == "top"} == set(ws.ALGOS)
    assert {c.algo for c, _ in ALL if c.pattern is not None} == set(ws.ALGOS)


@pytest.mark.parametrize("case", [c for c in ws.CASES if c.pattern is not None], ids=ws.case_id)
def test_small_segment_cases_have_a_chunk_over_many_segments(case):
    """The case's pattern input has a chunk of 4 segments or more: segments
    that hold no chunk start (walk.hpp: E = X)."""
    p = ws.params(case.algo, *ws.sizes_of(case), cfg=case.cfg)
    r = ws.ref(case, "pattern")
    assert int(r[:, 1].max()) >= 4 << p.seg_log2, (ws.case_id(case), int(r[:, 1].max()), p.seg_log2)
    assert int(r[:, 1].sum()) == case.n
    # and the zero-region input crosses from content-defined cuts into the run and back
    z = ws.ref(case, "zero_region")
    assert int(z[:, 1].sum()) == case.n and len(z) > 3


def test_zero_inputs_cut_where_the_rules_say():
    """SeqCDC on zeros cuts only at max; Rabin and LeapCDC on zeros cut at min."""
    for c in ws.CASES:
        if c.group != "small" or c.algo not in ("seq", "rabin", "leap"):
            continue
        ln = ws.ref(c, "zeros")[:-1, 1]
        assert (ln == (c.max if c.algo == "seq" else c.min)).all(), ws.case_id(c)


def test_workspace_stays_under_a_gib():
    worst = 0
    for c, p in ALL:
        lens = [c.n] * len(ws.input_names(c)) + [0]
        worst = max(worst, ws.workspace_bytes(c.algo, p, ws.segments(p, lens), len(lens)))
    assert worst < 1 << 30, worst
    # the batch of more than 2^16 segments: small at its forced 4 KiB
    # segments, several GiB at LeapCDC's default 256 KiB ones
    lens = ws.big_batch_lengths()
    for algo in ws.ALGOS:
        p = ws.params(algo, *ws.BIG[algo][0], walk=ws.BIG_WALK)
        assert ws.workspace_bytes(algo, p, ws.segments(p, lens), len(lens)) < 1 << 30, algo
    p = ws.params("leap", *ws.BIG["leap"][0])
    assert ws.workspace_bytes("leap", p, ws.segments(p, lens), len(lens)) > 3 << 30


def test_big_batch_shape():
    lens = ws.big_batch_lengths()
    p = ws.params("rabin", *ws.BIG["rabin"][0], walk=ws.BIG_WALK)
    assert (p.seg_log2, p.warm, p.nbm) == (12, 2 * ws.BIG["rabin"][0][1], 1)
    a = np.array(lens)
    assert len(lens) == ws.BIG_STREAMS and (a[::97] == 0).all() and (a[-5:] == 0).all()
    assert 250 <= int((a >= 20000).sum()) <= ws.BIG_LONG and int(a.max()) <= 200000
    assert ((a <= 200) | (a >= 20000)).all()
    assert ws.segments(p, lens) > ws.FINISH_MAX + 256 * 4            # the prefix carry loop: more than 256 block sums
    for want in (ws.FINISH_MAX, ws.FINISH_MAX + 1):
        t = ws.trim_to_segments(lens, 12, want)
        assert ws.segments(p, t) == want and t[:-1] == lens[:len(t) - 1]


@pytest.mark.parametrize("algo", ws.ALGOS)
def test_big_batch_settles_in_the_first_round(algo):
    """The model of the schedule for the batch of more than 2^16 segments: at
    the rule's sizes and bytes (ws.BIG) the first fix-up round changes no exit,
    so the engine is to take the gated output behind it; and the 2-avg warm-up
    does leave that round segments to walk again."""
    sizes, kind = ws.BIG[algo]
    lens, pieces = ws.big_batch(kind)
    case = ws.big_case(algo)
    p = ws.params(algo, *sizes, walk=ws.BIG_WALK)
    assert sizes[2] < 1 << p.seg_log2 and (1 << p.seg_log2) % sizes[2] and p.cap <= 514
    again = changed = 0
    for n, d in zip(lens, pieces):
        if n >= 20000:
            a, c = ws.rounds_settle_at_once(case, d, p.seg_log2, p.warm)
            again, changed = again + a, changed + c
    assert changed == 0 and again > 0, (algo, again, changed)


@pytest.mark.parametrize("case", ws.WRITE_CASES, ids=ws.case_id)
def test_write_inputs_end_in_max_cuts(case):
    data, whole = ws.write_inputs(case)["random_then_run"]
    assert int(whole[:, 1].sum()) == case.n == len(data)
    assert case.max == 16 << 20 and case.max in whole[:-1, 1].tolist()


def _refused(make):
    import chunkfs_amd as c
    with pytest.raises(c.CdcError) as ei:
        make(c)
    assert ei.value.code == -1          # CDC_EINVAL, before any device call
    return str(ei.value)


@pytest.mark.parametrize("algo,sizes", [
    ("rabin", (0, 10, 20)), ("ultra", (0, 10, 20)), ("leap", (0, 10, 20)), ("seq", (0, 10, 20)),   # min == 0
    ("rabin", (100, 50, 200)), ("seq", (100, 50, 200)), ("ultra", (100, 50, 200)),                 # min > avg
    ("rabin", (10, 300, 200)), ("leap", (64, 300, 200)), ("seq", (10, 300, 200)),                  # avg > max
    ("ultra", (7, 8, 16)), ("leap", (31, 64, 128)), ("rabin", (1, 1, 2)),
])
def test_validate_refusals_name_the_rule(algo, sizes):
    def make(c):
        cls = {"rabin": c.RabinChunker, "ultra": c.UltraChunker, "leap": c.LeapChunker}.get(algo)
        return cls(c.SizeParams(*sizes)) if cls else c.SeqChunker(0, c.SizeParams(*sizes))
    msg = _refused(make)
    assert "need 0 < min <= avg <= max" in msg
    assert "UltraCDC min >= 8" in msg and "LeapCDC min >= 32" in msg and "RabinCDC avg >= 2" in msg


@pytest.mark.parametrize("sizes,window", [((0, 10, 20), 4), ((100, 50, 200), 4), ((10, 300, 200), 4)])
def test_validate_refuses_ae_size_orderings(sizes, window):
    msg = _refused(lambda c: c.AeChunker(c.SizeParams(*sizes), window=window))
    assert "need 0 < min <= avg <= max" in msg


@pytest.mark.parametrize("sizes,window", [((16, 64, 256), 256), ((16, 64, 256), 0xFFFFFFFF), ((3, 3, 3), 3)])
def test_validate_refuses_ae_window_past_max(sizes, window):
    msg = _refused(lambda c: c.AeChunker(c.SizeParams(*sizes), window=window))
    assert "window + 1 <= max" in msg
