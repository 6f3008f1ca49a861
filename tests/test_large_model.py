"""What tests/test_gpu_large.py stands on, checked without a GPU: the two
properties of the CPU oracle that make a 4 GiB chunk list verifiable piece by
piece (restart and prefix stability, tests/large_model.py), for every rule
verified that way and for tests/ae_model.py; and the verifier itself: it
accepts the oracle's own list, compares every row exactly once, and rejects
each planted fault naming the piece that holds it.

And what tests/test_gpu_large_later.py stands on: blake2sp_rows against
blake2sp_model.oracle, pack_index against pack_model.pack byte for byte, the
delta closed forms against delta_model.delta on the same edits scaled down (the
line parametrised), the device-side comparison of a pack's data section on CPU
tensors, and the power condition: at N_BIG every expectation holds a value
>= 2^32 in the field its case is named for and changes when that field is cut
to 32 bits.
"""
import numpy as np
import pytest

import ae_model
import large_model as lm
import oracle

SIZES = (4096, 8192, 16384)
N = (16 << 20) + 4099
PIECES = 8

RULES = {
    "fast": lambda d: oracle.fastcdc(d, *SIZES),
    "rabin": lambda d: oracle.cdc("rabin", d, *SIZES),
    "ultra": lambda d: oracle.cdc("ultra", d, *SIZES),
    "leap": lambda d: oracle.cdc("leap", d, *SIZES),
    "seq": lambda d: oracle.cdc("seq", d, *SIZES),
    "seq_decreasing": lambda d: oracle.cdc("seq", d, *SIZES, seqcfg=(1, 5, 50, 256)),
}
_memo = {}


def data():
    if "d" not in _memo:
        d = oracle.splitmix64_bytes(N, 2032)
        d.setflags(write=False)
        _memo["d"] = d
    return _memo["d"]


def ref(rule):
    if rule not in _memo:
        r = RULES[rule](data())
        r.setflags(write=False)
        _memo[rule] = r
    return _memo[rule]


def fetch(a, b):
    return data()[a:b]


def shifted(rows, by):
    return np.asarray(rows, dtype=np.uint64).reshape(-1, 2) + np.array([by, 0], dtype=np.uint64)


# ---- the two properties -----------------------------------------------------------

@pytest.mark.parametrize("rule", list(RULES))
def test_oracle_restarts_at_any_cut(rule):
    r, d = ref(rule), data()
    assert len(r) > 1000
    for k in [1, 2, len(r) // 7, len(r) // 3, len(r) // 2 + 1, len(r) - 40, len(r) - 1]:
        c = int(r[k, 0])
        assert np.array_equal(shifted(RULES[rule](d[c:]), c), r[k:]), (rule, k, c)


@pytest.mark.parametrize("rule", list(RULES))
def test_oracle_prefix_is_stable(rule):
    r, d = ref(rule), data()
    ends = r[:, 0] + r[:, 1]
    for m in [SIZES[2] + 1, 100003, (1 << 20) + 1, (5 << 20) - 1, (12 << 20) + 4097, N - 1]:
        p = RULES[rule](d[:m])
        k = int(((p[:, 0] + p[:, 1]) <= m - SIZES[2]).sum())
        assert np.array_equal(p[:k], r[:k]), (rule, m)
        # ... and the stable part is all of the true list that ends there
        assert k == int((ends <= m - SIZES[2]).sum()), (rule, m)


AE_N = (3 << 19) + 77


def _ae(d):
    return ae_model.chunk_array(d, *SIZES)


def test_ae_model_restarts_and_prefix_is_stable():
    d = oracle.splitmix64_bytes(AE_N, 2033)
    r = _ae(d)
    assert len(r) > 100
    for k in [1, len(r) // 3, len(r) - 2]:
        c = int(r[k, 0])
        assert np.array_equal(shifted(_ae(d[c:]), c), r[k:]), k
    ends = r[:, 0] + r[:, 1]
    for m in [SIZES[2] + 5, 300001, (1 << 20) + 3]:
        p = _ae(d[:m])
        k = int(((p[:, 0] + p[:, 1]) <= m - SIZES[2]).sum())
        assert np.array_equal(p[:k], r[:k]) and k == int((ends <= m - SIZES[2]).sum()), m


# ---- the verifier accepts --------------------------------------------------------

def test_constants():
    assert lm.LINE == 1 << 32 and lm.N_BIG == (1 << 32) + (16 << 20) + 4099
    assert lm.EDGE_LENS == (lm.LINE - 1, lm.LINE, lm.LINE + 1)
    for m in (16, 65536, 1 << 12, 1 << 22):          # ragged: no multiple of a span or of a segment
        assert lm.N_BIG % m
    assert 1 <= lm.pool_size() <= 16 and lm.pool_size(3) == 3


def test_piece_bounds_are_offsets_of_the_list():
    r = ref("fast")
    b = lm.piece_bounds(r, N, PIECES)
    assert len(b) == PIECES and b[0] == 0 and all(x < y for x, y in zip(b, b[1:]))
    step = -(-N // PIECES)
    offs = r[:, 0]
    for i, c in enumerate(b[1:], 1):
        assert c in offs and c >= i * step and int(offs[offs < c][-1]) < i * step
    assert lm.piece_bounds(np.zeros((0, 2), dtype=np.uint64), 0, PIECES) == [0]
    assert lm.piece_bounds(r[:1], int(r[0, 1]), PIECES) == [0]


@pytest.mark.parametrize("rule", list(RULES))
def test_verifier_accepts_the_oracles_list_and_compares_every_row(rule):
    r = ref(rule)
    for pieces in (1, PIECES, 61, 5000):
        rep = lm.verify_by_pieces(r, N, fetch, RULES[rule], SIZES[2], pieces=pieces)
        assert rep.compared == len(r), (rule, pieces)
        assert rep.pieces == len(rep.bounds) and rep.bounds == lm.piece_bounds(r, N, pieces)
        assert rep.pieces == pieces or pieces == 5000
    assert lm.verify_by_pieces(r, N, fetch, RULES[rule], SIZES[2], pieces=PIECES, threads=1).compared == len(r)


def test_verifier_on_short_and_empty_lists():
    d = data()
    for n in (0, 1, SIZES[0], SIZES[2] + 1):
        r = RULES["fast"](d[:n])
        assert lm.verify_by_pieces(r, n, fetch, RULES["fast"], SIZES[2], pieces=PIECES).compared == len(r)
    with pytest.raises(lm.Mismatch):
        lm.verify_by_pieces(np.zeros((0, 2), dtype=np.uint64), 5, fetch, RULES["fast"], SIZES[2])


def test_explicit_bounds_must_be_offsets_of_the_list():
    r = ref("rabin")
    good = [0, int(r[500, 0]), int(r[900, 0])]
    assert lm.verify_by_pieces(r, N, fetch, RULES["rabin"], SIZES[2], bounds=good).compared == len(r)
    with pytest.raises(lm.Mismatch, match=f"boundary {good[1] + 1} is not an offset") as e:
        lm.verify_by_pieces(r, N, fetch, RULES["rabin"], SIZES[2], bounds=[0, good[1] + 1, good[2]])
    assert e.value.piece == 1 and e.value.offset == good[1] + 1


# ---- the verifier rejects --------------------------------------------------------

def _piece_rows(r):
    """Row index of every piece's first chunk, for the true list."""
    offs = [int(x) for x in r[:, 0]]
    return [offs.index(c) for c in lm.piece_bounds(r, N, PIECES)]


def _mid(r, piece):
    rows = _piece_rows(r)
    return (rows[piece] + rows[piece + 1]) // 2


def move_cut(r, j, by=1):
    """The cut between rows j - 1 and j, `by` bytes later."""
    g = np.array(r)
    g[j - 1, 1] += by
    g[j, 0] += by
    g[j, 1] -= by
    return g


def drop_cut(r, j):
    g = np.array(r)
    g[j - 1, 1] += g[j, 1]
    return np.delete(g, j, axis=0)


def split_chunk(r, j):
    o, ln = int(r[j, 0]), int(r[j, 1])
    return np.concatenate([r[:j], np.array([[o, ln // 2], [o + ln // 2, ln - ln // 2]], dtype=np.uint64), r[j + 1:]])


def wrap_from(r, j, line):
    g = np.array(r)
    g[j:, 0] %= np.uint64(line)
    return g


def _rejects(rule, got, piece, offset, pieces=PIECES):
    with pytest.raises(lm.Mismatch) as e:
        lm.verify_by_pieces(got, N, fetch, RULES[rule], SIZES[2], pieces=pieces, what=rule)
    assert e.value.piece == piece, str(e.value)
    assert e.value.offset == offset, str(e.value)
    assert f"{rule}: piece {piece}:" in str(e.value)
    return str(e.value)


@pytest.mark.parametrize("rule", ["fast", "rabin", "seq"])
def test_rejects_a_cut_moved_by_one_byte(rule):
    r = ref(rule)
    for piece in (0, 3, PIECES - 1):
        j = _mid(r, piece) if piece < PIECES - 1 else len(r) - 3
        msg = _rejects(rule, move_cut(r, j), piece, int(r[j - 1, 0]))
        assert str([int(r[j - 1, 0]), int(r[j - 1, 1]) + 1]) in msg and str([int(x) for x in r[j - 1]]) in msg


@pytest.mark.parametrize("rule", ["fast", "ultra"])
def test_rejects_a_dropped_cut(rule):
    r = ref(rule)
    j = _mid(r, 5)
    _rejects(rule, drop_cut(r, j), 5, int(r[j - 1, 0]))


@pytest.mark.parametrize("rule", ["fast", "leap"])
def test_rejects_a_split_chunk(rule):
    r = ref(rule)
    j = _mid(r, 2)
    _rejects(rule, split_chunk(r, j), 2, int(r[j, 0]))


@pytest.mark.parametrize("rule", ["fast", "rabin"])
def test_rejects_offsets_wrapped_at_a_line(rule):
    """What a 32-bit wrap looks like, with 4 MiB standing in for 2^32: from
    some chunk on the offsets are reduced modulo the line."""
    r, line = ref(rule), 1 << 22
    j = _mid(r, 6)
    assert int(r[j, 0]) > 3 * line
    msg = _rejects(rule, wrap_from(r, j, line), 6, int(r[j, 0]) % line)
    assert str([int(x) for x in r[j]]) in msg
    # ... and a wrap that begins exactly at a boundary chunk
    j = _piece_rows(r)[4]
    _rejects(rule, wrap_from(r, j, line), 3, int(r[j, 0]) % line)


@pytest.mark.parametrize("rule", ["fast", "seq_decreasing"])
def test_rejects_a_list_cut_short(rule):
    r = ref(rule)
    j = _mid(r, 6)
    _rejects(rule, r[:j], 6, int(r[j, 0]))
    _rejects(rule, r[:-1], PIECES - 1, int(r[-1, 0]))
    _rejects(rule, r[:_piece_rows(r)[4]], 3, int(r[_piece_rows(r)[4], 0]))   # short by whole pieces


@pytest.mark.parametrize("rule", ["fast", "rabin", "ultra", "leap", "seq"])
def test_rejects_a_fault_exactly_at_a_piece_boundary(rule):
    r = ref(rule)
    kb = _piece_rows(r)[4]
    # the boundary chunk itself is one byte long: piece 4 starts with it
    _rejects(rule, move_cut(r, kb + 1), 4, int(r[kb, 0]))
    # the boundary itself is one byte late: piece 3 ends with the chunk that grew
    _rejects(rule, move_cut(r, kb), 3, int(r[kb - 1, 0]))
    # the boundary chunk is missing: the list jumps over it
    g = np.delete(np.array(r), kb, axis=0)
    with pytest.raises(lm.Mismatch) as e:
        lm.verify_by_pieces(g, N, fetch, RULES[rule], SIZES[2], pieces=PIECES)
    assert e.value.piece in (3, 4), str(e.value)


def test_rejects_a_boundary_no_chunk_ends_at():
    """Equal rows on both sides of a boundary that is no cut: the last chunk of
    the piece runs past it (a list that does not tile)."""
    r = ref("fast")
    kb = _piece_rows(r)[4]
    g = np.array(r)
    g[kb:, 0] -= np.uint64(1)                   # every later offset one byte down: rows of piece 4 on all differ,
    with pytest.raises(lm.Mismatch) as e:       # but piece 3's rows are the oracle's and its end is not a cut
        lm.verify_by_pieces(g, N, fetch, RULES["fast"], SIZES[2], pieces=PIECES)
    assert e.value.piece == 3 and "is not a cut of the oracle's list" in str(e.value)
    assert e.value.offset == int(r[kb, 0]) - 1


# ---- windows and shorter lengths -------------------------------------------------

def test_verify_window_accepts_and_rejects():
    d = oracle.splitmix64_bytes(AE_N, 2033)
    r = _ae(d)

    def f(a, b):
        return d[a:b]

    total = 0
    for at, length in [(0, 300000), (400001, 1 << 18), (AE_N - 200000, 1 << 20)]:
        c, k = lm.verify_window(r, AE_N, f, _ae, SIZES[2], at, length)
        assert c >= at and c in r[:, 0] and k > 10
        total += k
    j = int(np.searchsorted(r[:, 0], np.uint64(400001))) + 5
    with pytest.raises(lm.Mismatch) as e:
        lm.verify_window(move_cut(r, j), AE_N, f, _ae, SIZES[2], 400001, 1 << 18)
    assert e.value.offset == int(r[j - 1, 0])
    with pytest.raises(lm.Mismatch):            # the list ends inside a window that reaches the end
        lm.verify_window(r[:-1], AE_N, f, _ae, SIZES[2], AE_N - 200000, 1 << 20)
    with pytest.raises(lm.Mismatch, match="no cut at or after"):
        lm.verify_window(r, AE_N, f, _ae, SIZES[2], AE_N, 10)


@pytest.mark.parametrize("rule", ["fast", "rabin", "seq"])
def test_verify_against_longer(rule):
    r, d = ref(rule), data()
    for length in [(8 << 20) - 1, 8 << 20, (8 << 20) + 1]:
        g = RULES[rule](d[:length])
        assert lm.verify_against_longer(g, length, r, fetch, RULES[rule], SIZES[2]) == len(g)
        with pytest.raises(lm.Mismatch):
            lm.verify_against_longer(move_cut(g, 100), length, r, fetch, RULES[rule], SIZES[2])
        with pytest.raises(lm.Mismatch):
            lm.verify_against_longer(move_cut(g, len(g) - 1), length, r, fetch, RULES[rule], SIZES[2])
        with pytest.raises(lm.Mismatch):
            lm.verify_against_longer(g[:-1], length, r, fetch, RULES[rule], SIZES[2])


def test_sha256_rows_equals_a_plain_loop():
    import hashlib
    r, d = ref("fast")[:700], data()
    rows = np.concatenate([r, np.array([[5, 0], [0, 1], [N - 3, 3]], dtype=np.uint64)])
    want = [hashlib.sha256(d[int(o):int(o) + int(ln)].tobytes()).digest() for o, ln in rows]
    for threads in (None, 1, 3):
        got = lm.sha256_rows(d, rows, threads)
        assert got.shape == (len(rows), 32) and [bytes(x) for x in got] == want
    assert lm.sha256_rows(d, np.zeros((0, 2), dtype=np.uint64)).shape == (0, 32)


# ---- what test_gpu_large_later.py expects -----------------------------------------

def test_blake2sp_rows_equals_the_oracle():
    import blake2sp_model as bm
    d = data()
    edges = [0, 1, 63, 64, 65, 447, 448, 449, 511, 512, 513, 575, 576, 1023, 1024, 1025, 4095, 4096, 4097, 70001]
    rows = np.concatenate([ref("fast")[:200], np.array([[7 + 3 * i, n] for i, n in enumerate(edges)], dtype=np.uint64),
                           np.array([[N - 3, 3], [12345, (1 << 20) + 77]], dtype=np.uint64)])
    want = [bm.oracle(d[int(o):int(o) + int(ln)].tobytes()) for o, ln in rows]
    for threads in (None, 1, 3):
        got = lm.blake2sp_rows(d, rows, threads)
        assert got.shape == (len(rows), 32) and [bytes(x) for x in got] == want
    assert lm.blake2sp_rows(d, np.zeros((0, 2), dtype=np.uint64)).shape == (0, 32)
    for msg, hexd in bm.KNOWN.items():
        assert lm.blake2sp_one(np.frombuffer(msg, dtype=np.uint8)).hex() == hexd


def _model_file(content, chunks):
    import gc_model as gm
    files = gm.Files()
    h = files.create("f")
    if len(chunks):
        files.append(h, content, np.asarray(chunks, dtype=np.uint64).reshape(-1, 2))
    return files, h


def _pack_tilings():
    import pack_model as pm
    d = data()
    out = {label: v for label, v in pm.shapes().items()}                   # 0 and 1 spans, padding lengths, repeats
    out["fastcdc"] = (d[:300001], RULES["fast"](d[:300001]))
    block = d[:4096]
    out["repeats between"] = (np.concatenate([block, d[5000:5777], block, block, d[9000:9001]]),
                              pm.tiling([4096, 777, 4096, 4096, 1]))
    return out


@pytest.mark.parametrize("label", ["empty", "one span", "2049 spans", "padding lengths", "length-0 spans",
                                   "heavy duplication", "fastcdc", "repeats between"])
def test_pack_index_equals_the_pack_model(label):
    import pack_model as pm
    content, chunks = _pack_tilings()[label]
    files, h = _model_file(content, chunks)
    blob, st = pm.pack(files, h)
    digests = np.frombuffer(b"".join(files.hashes(h)), dtype=np.uint8).reshape(-1, 32)
    x = lm.pack_index(chunks, digests)
    assert x.layout == pm.layout(len(chunks), x.n_chunks, x.data_bytes)
    assert x.index.tobytes() == blob[:x.layout["data"]]
    assert len(blob) == x.layout["total"] == st["pack_bytes"]
    assert (st["spans"], st["chunks"], st["chunk_bytes"], st["file_size"], st["external_spans"]) == \
        (len(chunks), x.n_chunks, x.chunk_bytes, x.file_size, 0)
    # ... and the data section is what the index says: chunk k at chunk_off[k], zeros after it
    body = np.frombuffer(blob, dtype=np.uint8)[x.layout["data"]:]
    assert body.size == x.data_bytes
    for k in range(x.n_chunks):
        o, ln = (int(v) for v in np.asarray(chunks, dtype=np.uint64).reshape(-1, 2)[int(x.chunk_span[k])])
        a, b = int(x.chunk_off[k]), int(x.chunk_off[k + 1])
        assert np.array_equal(body[a:a + ln], content[o:o + ln]) and not body[a + ln:b].any()


def test_pack_data_mismatch_compares_every_byte():
    """The device-side comparison of a pack's data section, here on CPU tensors
    and in slabs that end inside chunks and inside padding."""
    import torch
    import pack_model as pm
    content, chunks = _pack_tilings()["fastcdc"]
    chunks = np.concatenate([chunks[:-1], [[int(chunks[-1, 0]), 5]], [[int(chunks[-1, 0]) + 5, int(chunks[-1, 1]) - 5]]])
    files, h = _model_file(content, chunks.astype(np.uint64))
    blob, _ = pm.pack(files, h)
    x = lm.pack_index(chunks, np.frombuffer(b"".join(files.hashes(h)), dtype=np.uint8).reshape(-1, 32))
    body = np.frombuffer(blob, dtype=np.uint8)[x.layout["data"]:].copy()
    buf = torch.from_numpy(content.copy())
    for slab in (1 << 20, 4099, 1000):
        assert lm.pack_data_mismatch(torch.from_numpy(body), buf, chunks, x.chunk_span, x.chunk_off, slab) is None
    k = x.n_chunks - 2                                        # the 5-byte chunk: 11 bytes of padding behind it
    a = int(x.chunk_off[k])
    assert int(x.chunk_off[k + 1]) - a == 16
    for at in (0, 4098, 4099, a + 4, a + 5, a + 15, a + 16, body.size - 1):
        bad = body.copy()
        bad[at] ^= 1
        for slab in (1 << 20, 4099):
            assert lm.pack_data_mismatch(torch.from_numpy(bad), buf, chunks, x.chunk_span, x.chunk_off, slab) == at
    moved = torch.from_numpy(np.roll(content, 1))             # the right pack, the wrong source
    assert lm.pack_data_mismatch(torch.from_numpy(body), moved, chunks, x.chunk_span, x.chunk_off) == 0


def test_common_prefix_and_suffix():
    d = data()[:300000]
    for n in (0, 1, 65535, 65536, 65537, 200001):
        x = d.copy()
        x[n] ^= 1
        assert lm.common_prefix(d, x) == n == lm.common_prefix(x, d[:250000])
        y = d.copy()
        y[y.size - 1 - n] ^= 1
        assert lm.common_suffix(d, y) == n == lm.common_suffix(y[1000:], d)
    assert lm.common_prefix(d, d[:70000]) == 70000 == lm.common_suffix(d, d[-70000:])
    assert lm.common_prefix(d, d[:0]) == 0 == lm.common_suffix(d[:0], d)


def test_constants_read_from_the_sources():
    assert lm.csrc_const("kDlMaxBlocks", "delta.hip") == 1 << 18
    assert lm.csrc_const("kDeltaTile", "delta_plan.hpp") == 4096
    assert lm.delta_tiles(0) == 0 and lm.delta_tiles(1) == 1 and lm.delta_tiles(4096) == 1 and lm.delta_tiles(4097) == 2
    assert lm.delta_tiles(lm.LINE + 5) > lm.csrc_const("kDlMaxBlocks", "delta.hip")
    with pytest.raises(KeyError):
        lm.csrc_const("kNoSuchConstant", "delta.hip")


DELTA_TAIL = (16 << 10) + 99      # what N_BIG has past the line, scaled down


def _delta_setup(line):
    import delta_model as dl
    n = line + DELTA_TAIL
    d = dl.ModelDriver("fast")
    content = dl.rand(7000 + line, n)
    a = d.file("a", content)
    return dl, d, content, a, n


def _ops_of(r):
    return [tuple(int(x) for x in o) for o in r["ops"]]


@pytest.mark.parametrize("line", [40000, 1 << 16, 70001])
def test_delta_closed_forms_equal_the_delta_model(line):
    dl, d, content, a, n = _delta_setup(line)
    assert lm.DELTA_LIT == dl.LIT
    # (i) an insert past the line
    p, ins = line + 99, dl.rand(1, 7)
    ins[0], ins[-1] = content[p] ^ 1, content[p - 1] ^ 1
    b = d.clone("a", "ins")
    d.splice(b, p, 0, ins)
    r = d.delta(a, b)
    assert _ops_of(r) == lm.delta_insert(n, p, 7) and r["regions"] == 1 and r["bytes_literal"] == 7
    t = d.delta(a, b, True)
    lit = [o for o in t["ops"] if o[2] == dl.LIT]
    assert len(lit) == 1 and lit[0][0] <= p and p + 7 <= lit[0][0] + lit[0][1] == lit[0][0] + r["bytes_literal_tables"]
    # (ii), (iii) the head dropped, and put back
    cut = line + 5
    e = lm.common_prefix(content[cut:], content)
    b = d.clone("a", "tail")
    d.splice(b, 0, cut, None)
    assert np.array_equal(d.content(b), content[cut:])
    assert _ops_of(d.delta(a, b)) == lm.delta_drop_head(n, cut, e)
    r = d.delta(b, a)
    assert _ops_of(r) == lm.delta_restore_head(n, cut, e) and r["bytes_literal"] == cut - e
    # (iv) the first bytes once more at the end: every slot of theirs twice, `n` apart
    import splice_model as spm
    b = d.clone("a", "dup")
    head = content[:4096]
    d.m.append(b, head, spm.chunk("fast", head))
    twice = [sp.hash for sp in d.m._spans(b)]
    assert twice.count(twice[0]) == 2
    assert _ops_of(d.delta(b, b)) == lm.delta_self(n + 4096)
    # (v) truncated, and grown back
    b = d.clone("a", "cut")
    d.splice(b, line + 1, n - line - 1, None)
    f = lm.common_suffix(content, content[:line + 1])
    assert _ops_of(d.delta(a, b)) == lm.delta_truncate(n, line + 1)
    assert _ops_of(d.delta(b, a)) == lm.delta_extend(n, line + 1, f)


def test_delta_closed_forms_with_shared_edges():
    """e and f are not always 0: contents built so that the searches do match some bytes."""
    import delta_model as dl
    line = 30000
    n = line + DELTA_TAIL
    content = dl.rand(7100, n)
    cut = line + 5
    content[cut:cut + 3] = content[:3]                   # A[cut:] opens like A
    content[cut + 3] = content[3] ^ 1
    content[n - 2:] = content[line - 1:line + 1]         # A ends like A[:line + 1]
    content[n - 3] = content[line - 2] ^ 1
    d = dl.ModelDriver("fast")
    a = d.file("a", content)
    assert lm.common_prefix(content[cut:], content) == 3 and lm.common_suffix(content, content[:line + 1]) == 2
    b = d.clone("a", "tail")
    d.splice(b, 0, cut, None)
    assert _ops_of(d.delta(a, b)) == lm.delta_drop_head(n, cut, 3)
    assert _ops_of(d.delta(b, a)) == lm.delta_restore_head(n, cut, 3)
    b = d.clone("a", "cut")
    d.splice(b, line + 1, n - line - 1, None)
    assert _ops_of(d.delta(b, a)) == lm.delta_extend(n, line + 1, 2)


def test_the_large_cases_have_power():
    """For every case of test_gpu_large_later.py, the expectation at the real
    N_BIG holds a value >= 2^32 in the field the case is named for, and the same
    expectation with that field cut to 32 bits is another one: a uint32_t in
    that place cannot pass."""
    LINE, N_BIG = lm.LINE, lm.N_BIG
    LIT = lm.DELTA_LIT
    # packs: chunk_off, data_bytes, total_bytes and the layout's data offset + chunk_off.  A tiling of N_BIG
    # with lengths in the 16 / 64 / 256 KiB list's range stands in for the real list (the GPU case asserts
    # the same on the real one).
    rng = np.random.default_rng(5)
    lens = rng.integers(16384, 262145, 40000).astype(np.uint64)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), N_BIG))]
    lens = np.append(lens, np.uint64(N_BIG - int(lens.sum())))
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    rows = np.stack([offs, lens], axis=1)
    digests = np.arange(len(rows) * 4, dtype="<u8").view(np.uint8).reshape(-1, 32)      # distinct
    x = lm.pack_index(rows, digests)
    assert x.n_chunks == len(rows) and x.file_size == N_BIG
    assert int(x.chunk_off[-1]) == x.data_bytes >= LINE and x.layout["total"] >= LINE
    assert lm.masked32(x.chunk_off) != [int(v) for v in x.chunk_off]
    assert lm.masked32([x.data_bytes, x.layout["total"]]) != [x.data_bytes, x.layout["total"]]
    assert (x.data_bytes // 16384 + x.n_chunks) > 1 << 18              # the copy's tile bound, kStoreTile = 16 KiB
    # the batch write: the third request's base, in spans and bytes, lies past a 4 GiB request
    assert 1000 + N_BIG >= LINE

    def differs(ops, field):
        cut = [tuple(v & 0xFFFFFFFF if (i == field and v != LIT) else v for i, v in enumerate(o)) for o in ops]
        return cut != ops

    p, k = LINE + 99, 7
    ins = lm.delta_insert(N_BIG, p, k)
    assert max(a for _, _, a in ins if a != LIT) >= LINE and differs(ins, 2) and differs(ins, 0)
    d = LINE + 5
    drop = lm.delta_drop_head(N_BIG, d)
    assert all(a >= LINE for _, _, a in drop) and min(lm.delta_diagonals(drop)) >= LINE and differs(drop, 2)
    back = lm.delta_restore_head(N_BIG, d)
    assert lm.delta_literal(back) > LINE and min(lm.delta_diagonals(back)) < -LINE
    assert differs(back, 1) and differs(back, 0)
    assert lm.delta_literal(back) // 4096 > 1 << 18                    # more tiles than the edge pass has blocks
    whole = lm.delta_self(N_BIG + (1 << 20))
    assert whole[0][1] > N_BIG and differs(whole, 1)
    grow = lm.delta_extend(N_BIG, LINE + 1)
    assert grow[1][0] == LINE + 1 and differs(grow, 0) and differs(grow, 1)
    assert lm.delta_truncate(N_BIG, LINE + 1) == [(0, LINE + 1, 0)] and differs(lm.delta_truncate(N_BIG, LINE + 1), 1)
    assert min(lm.delta_diagonals(lm.delta_extend(N_BIG, LINE + 1, 3))) == LINE + 1 - N_BIG


def test_check_tiling():
    r = ref("fast")
    lm.check_tiling(r, N, SIZES[0], SIZES[2])
    lm.check_tiling(np.zeros((0, 2), dtype=np.uint64), 0, 1, 2)
    long = np.array(r)
    long[9, 1] += long[10, 1] + long[11, 1] + long[12, 1] + long[13, 1]     # five chunks in one: above max
    for bad in (np.delete(r, 50, axis=0), np.delete(long, [10, 11, 12, 13], axis=0), r[:-1], r[1:],
                wrap_from(r, 600, 1 << 22), split_chunk(split_chunk(split_chunk(r, 20), 20), 20)):    # a chunk under min
        with pytest.raises(AssertionError):
            lm.check_tiling(bad, N, SIZES[0], SIZES[2])
