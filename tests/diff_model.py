"""Python model of cdc_files_clone and cdc_files_diff_device (include/chunkfs_amd.h,
"Snapshots and diffs"), written for this repository over gc_model.Files, and the
cases the CPU and GPU suites share.

In the model a store slot is a digest: the store keeps one container per
digest, so "the same slot at the same file offset" is "the same digest at the
same span offset".

A case is a function of a driver.  ModelDriver runs it on the model alone
(tests/test_diff_model.py proves there that each case reaches the path it is
named for, and that the model equals a numpy mask over the two contents); the
GPU suite's driver runs the device layer beside the model and compares every
diff.  The assertions inside a case hold for both.
"""
import bisect

import numpy as np

import files_model as fm
import gc_model as gm
import splice_model as spm

EINVAL, ENOTFOUND, EEXIST = -1, fm.ENOTFOUND, fm.EEXIST
STATS = ("n_ranges", "bytes_differing", "bytes_compared", "bytes_shared", "pieces", "size_a", "size_b")
TILE = 4096


# ---- the model ---------------------------------------------------------------------------
def clone(files, src, dst):
    """cdc_files_clone: a deep copy of the span list; the store is not touched."""
    if src not in files.files:
        raise fm.ModelError(ENOTFOUND)
    if dst in files.files:
        raise fm.ModelError(EEXIST)
    files.files[dst] = [fm.Span(sp.hash, sp.offset, sp.len) for sp in files.files[src]]
    return len(files.files[dst])


def pieces(sa, sb):
    """[(start, end, span of A, span of B, shared)]: the distinct boundaries of
    both span lists inside (0, common) cut [0, common) into pieces; spans of
    length 0 hold no byte and add none."""
    size_a, size_b = sum(s.len for s in sa), sum(s.len for s in sb)
    common = min(size_a, size_b)
    if not common:
        return []
    full_a, full_b = [s for s in sa if s.len], [s for s in sb if s.len]
    starts_a, starts_b = [s.offset for s in full_a], [s.offset for s in full_b]
    cuts = sorted({s.offset for s in sa + sb if s.offset < common})
    out = []
    for k, x in enumerate(cuts):
        end = cuts[k + 1] if k + 1 < len(cuts) else common
        a, b = full_a[bisect.bisect_right(starts_a, x) - 1], full_b[bisect.bisect_right(starts_b, x) - 1]
        assert a.offset <= x and end <= a.offset + a.len and b.offset <= x and end <= b.offset + b.len
        out.append((x, end, a, b, a.hash == b.hash and a.offset == b.offset))
    return out


def runs(mask):
    """The maximal runs of a 0/1 array: [(offset, length)]."""
    m = np.concatenate([[0], np.asarray(mask, dtype=np.int8), [0]])
    d = np.diff(m)
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return [(int(s), int(e - s)) for s, e in zip(starts, ends)]


def mask_ranges(a, b):
    """The brute-force answer from the two contents alone."""
    common, most = min(a.size, b.size), max(a.size, b.size)
    mask = np.ones(most, dtype=np.int8)
    mask[:common] = a[:common] != b[:common]
    return runs(mask)


def diff(files, ha, hb, tables_only=False):
    """cdc_files_diff_device: {"ranges": [(offset, length)], and STATS}."""
    sa, sb = files._spans(ha), files._spans(hb)
    a, b = files.read_complete(ha), files.read_complete(hb)
    common, most = min(a.size, b.size), max(a.size, b.size)
    mask = np.ones(most, dtype=np.int8)
    ps = pieces(sa, sb)
    compared = 0
    for x, end, _, _, shared in ps:
        if shared:
            mask[x:end] = 0
        else:
            compared += end - x
            if not tables_only:
                mask[x:end] = a[x:end] != b[x:end]
    r = runs(mask)
    return {"ranges": r, "n_ranges": len(r), "bytes_differing": int(mask.sum()),
            "bytes_compared": 0 if tables_only else compared, "bytes_shared": common - compared, "pieces": len(ps),
            "size_a": a.size, "size_b": b.size}


class ModelDriver:
    """The cases' driver on the model alone.  Handles are the model's."""

    def __init__(self, name="fast"):
        self.name, self.m = name, gm.Files()

    def file(self, fname, data, chunks=None):
        """A file holding `data`: cut by the driver's chunker, or by hand."""
        h = self.m.create(fname)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if chunks is None:
            chunks = spm.chunk(self.name, data)
        if len(chunks):
            self.m.append(h, data, np.asarray(chunks, dtype=np.uint64).reshape(-1, 2))
        return h

    def clone(self, src, dst):
        clone(self.m, src, dst)
        return self.m.open(dst)

    def splice(self, h, offset, rem, ins):
        return spm.splice(self.m, h, self.name, offset, rem, ins)

    def content(self, h):
        return self.m.read_complete(h)

    def table(self, h):
        return spm.table(self.m, h)

    def diff(self, a, b, tables_only=False):
        return diff(self.m, a, b, tables_only)


# ---- data ---------------------------------------------------------------------------------
def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def tiling(lengths):
    lengths = np.asarray(lengths, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.uint64) if len(lengths) else lengths
    return np.stack([offs, lengths], axis=1)


def flipped(data, positions):
    out = data.copy()
    out[np.asarray(positions, dtype=np.int64)] ^= 0xFF
    return out


# ---- the cases ------------------------------------------------------------------------------
# Each returns {label: result of d.diff}; what it asserts is what its name promises.
def case_nothing_to_read(d):
    data = rand(11, 96 << 10)
    a = d.file("a", data)
    b = d.clone("a", "b")
    out = {"clone": d.diff(b, a), "self": d.diff(a, a)}
    mid = data.size // 2
    d.splice(b, mid, 4096, data[mid:mid + 4096])  # the bytes already there: the same chunks, the same slots
    out["same_bytes"] = d.diff(a, b)
    for r in out.values():
        assert r["ranges"] == [] and r["bytes_compared"] == 0 and r["bytes_shared"] == data.size
    return out


def case_one_edit(d, n, tables_only=False):
    data = rand(12, 96 << 10)
    a = d.file("a", data)
    b = d.clone("a", "b")
    mid = data.size // 2 + 3
    d.splice(b, mid, n, data[mid:mid + n] ^ 0xFF)
    r = d.diff(a, b, tables_only)
    touched = r["size_a"] - r["bytes_shared"]
    assert n <= touched <= n + 6 * 1024  # a few spans of at most 1024 bytes around the edit
    if tables_only:
        assert r["bytes_compared"] == 0 and len(r["ranges"]) == 1
        assert r["ranges"][0][0] <= mid and mid + n <= sum(r["ranges"][0]) and r["ranges"][0][1] == touched
    else:
        assert r["ranges"] == [(mid, n)] and r["bytes_compared"] == touched
    return {"edit": r}


EDGE_A = [100, 100, 100, 100, 100, 100]
EDGE_B = [100, 50, 150, 30, 70, 0, 100, 0, 0, 100]
EDGE_KINDS = {"a_only": 200, "b_only": 150, "common": 300, "common_with_empty_spans": 400, "b_only_2": 330}


def case_edges(d):
    """Hand-made tables over the same content; bytes flipped at -1, 0, +1 around
    each kind of boundary, alone and as runs across it."""
    data = rand(13, 600)
    a = d.file("a", data, tiling(EDGE_A))
    out = {}
    for kind, x in EDGE_KINDS.items():
        for label, pos in (("m1", [x - 1]), ("0", [x]), ("p1", [x + 1]), ("across", [x - 1, x]),
                           ("three", [x - 1, x, x + 1]), ("split", [x - 1, x + 1])):
            b = d.file(f"b_{kind}_{label}", flipped(data, pos), tiling(EDGE_B))
            r = d.diff(a, b)
            want = [(x - 1, 1), (x + 1, 1)] if label == "split" else [(pos[0], len(pos))]
            assert r["ranges"] == want, (kind, label, r["ranges"])
            assert r["pieces"] == 8
            out[f"{kind}_{label}"] = r
    return out


def case_two_ranges(d):
    """The last byte of span 3 and the first of span 5, span 4 shared between them."""
    assert d.name == "fixed"
    data = rand(14, 8 * 512)
    a = d.file("a", data)
    b = d.clone("a", "b")
    d.splice(b, 4 * 512 - 1, 1, data[4 * 512 - 1:4 * 512] ^ 0xFF)
    d.splice(b, 5 * 512, 1, data[5 * 512:5 * 512 + 1] ^ 0xFF)
    r = d.diff(a, b)
    assert r["ranges"] == [(4 * 512 - 1, 1), (5 * 512, 1)] and r["bytes_compared"] == 1024 and r["pieces"] == 8
    # the same edits with span 4 compared and equal: still two ranges, and with its every byte differing: one
    cut = [512, 512, 512, 512, 300, 212, 512, 512, 512]
    c = d.file("c", flipped(data, [4 * 512 - 1, 5 * 512]), tiling(cut))
    r2 = d.diff(a, c)
    assert r2["ranges"] == r["ranges"] and r2["bytes_shared"] == 5 * 512 and r2["pieces"] == 9
    e = d.file("e", flipped(data, range(4 * 512 - 1, 5 * 512 + 1)), tiling(cut))
    r3 = d.diff(a, e)
    assert r3["ranges"] == [(4 * 512 - 1, 514)]
    return {"shared_between": r, "compared_between": r2, "one_run": r3}


def case_tail(d):
    data = rand(15, 600)
    a = d.file("a", data, tiling([200, 200, 200]))
    out = {}
    b = d.file("b", flipped(data[:400], [399]), tiling([150, 250]))
    out["merges"] = d.diff(a, b)
    assert out["merges"]["ranges"] == [(399, 201)]
    c = d.file("c", data[:400], tiling([150, 250]))
    out["alone"] = d.diff(a, c)
    assert out["alone"]["ranges"] == [(400, 200)] and out["alone"]["bytes_compared"] == 400
    out["alone_swapped"] = d.diff(c, a)
    s = d.file("s", data[:400], tiling([200, 200]))  # the last piece shared: the tail is a range of its own
    out["after_shared"] = d.diff(a, s)
    assert out["after_shared"]["ranges"] == [(400, 200)] and out["after_shared"]["bytes_compared"] == 0
    e1, e2 = d.file("e1", data[:0]), d.file("e2", data[:0])
    z = d.file("z", data[:0], [[0, 0], [0, 0]])  # spans, and no byte
    out["empty_full"] = d.diff(e1, a)
    out["full_empty"] = d.diff(a, e1)
    out["zero_spans_full"] = d.diff(z, a)
    out["empty_empty"] = d.diff(e1, e2)
    out["empty_zero_spans"] = d.diff(e1, z)
    for k in ("empty_full", "full_empty", "zero_spans_full"):
        assert out[k]["ranges"] == [(0, 600)] and out[k]["pieces"] == 0
    assert out["empty_empty"]["ranges"] == [] and out["empty_zero_spans"]["ranges"] == []
    return out


ALIGN_L = (1, 15, 16, 17, 4095, 4096, 4097, 8193)


def case_alignment(d, L):
    """A is one span of L bytes, B other content cut [k, L - k], k = 1..17: every
    relative misalignment of the two sides (B's second span starts a container,
    A's byte k does not), either side as the one the tiles are aligned on, and
    every ragged head and tail."""
    data = rand(1600 + L, L)
    other = data.copy()
    rng = np.random.default_rng(1700 + L)
    other[rng.random(L) < 0.3] ^= 0x5A
    other[0] ^= 1
    if L > 1:
        other[-1] ^= 1
    a = d.file(f"a{L}", data, [[0, L]])
    out = {}
    for k in range(1, 18):
        if k > L:
            break
        b = d.file(f"b{L}_{k}", other, tiling([k, L - k]))
        out[f"ab{k}"] = d.diff(a, b)
        out[f"ba{k}"] = d.diff(b, a)
        assert out[f"ab{k}"]["bytes_compared"] == L and out[f"ab{k}"]["ranges"] == out[f"ba{k}"]["ranges"]
        assert out[f"ab{k}"]["pieces"] == (2 if k < L else 1)
    return out


def case_same_slot_shifted(d, tables_only=False):
    P, Q = np.zeros(300, np.uint8), rand(18, 100) | 1
    a = d.file("a", P, [[0, 300]])
    b = d.file("b", np.concatenate([Q, P]), tiling([100, 300]))
    r = d.diff(a, b, tables_only)
    X, Y = rand(19, 256), rand(20, 256)
    xyx = d.file("xyx", np.concatenate([X, Y, X]), tiling([256, 256, 256]))
    xxy = d.file("xxy", np.concatenate([X, X, Y]), tiling([256, 256, 256]))
    r2 = d.diff(xyx, xxy, tables_only)
    if tables_only:
        assert r["ranges"] == [(0, 400)] and r2["ranges"] == [(256, 512)]
        assert r["bytes_compared"] == 0 and r2["bytes_compared"] == 0
    else:
        # [100, 300) is slot P on both sides, 100 bytes apart: compared, and equal
        assert r["ranges"] == [(0, 100), (300, 100)] and r["bytes_compared"] == 300 and r["bytes_shared"] == 0
        assert r2["bytes_shared"] == 256 and r2["bytes_compared"] == 512
    return {"p_qp": r, "xyx_xxy": r2}


def case_dense(d):
    n = 16 << 10
    data = rand(21, n)
    a = d.file("a", data, [[0, n]])
    out = {}
    out["all"] = d.diff(a, d.file("inv", data ^ 0xFF, tiling([n // 2, n // 2])))
    assert out["all"]["ranges"] == [(0, n)]
    out["every_second"] = d.diff(a, d.file("alt", flipped(data, range(0, n, 2)), [[0, n]]))
    assert out["every_second"]["n_ranges"] == n // 2
    out["every_second_odd"] = d.diff(a, d.file("alt1", flipped(data, range(1, n, 2)), [[0, n]]))
    # one piece, both sides aligned: mask bit = file offset.  Runs on bits 0 and 63, over a word, over a tile.
    pos = list(range(64, 128)) + [191, 192] + [256, 319] + list(range(4000, 9000)) + [n - 64, n - 1]
    out["words"] = d.diff(a, d.file("words", flipped(data, pos), [[0, n]]))
    assert out["words"]["ranges"] == [(64, 64), (191, 2), (256, 1), (319, 1), (4000, 5000), (n - 64, 1), (n - 1, 1)]
    return out


COUNT_CASES = {1024: 2047, 2047: 2048, 2048: 2049, 2049: 4096, 5000: 4097}


def case_counts(d, n):
    """Two files of n and n + 1 spans of 16 - 64 bytes over contents that differ
    in COUNT_CASES[n] single bytes: about 2 n pieces."""
    rng = np.random.default_rng(2200 + n)
    la = rng.integers(16, 65, n)
    size = int(la.sum())
    data = rand(2300 + n, size)
    lb = np.concatenate([[8], la[:-1], [la[-1] - 8]])  # every boundary moved by 8: no piece is shared
    nr = COUNT_CASES[n]
    a = d.file("a", data, tiling(la))
    b = d.file("b", flipped(data, range(0, 2 * nr, 2)), tiling(lb))
    r = d.diff(a, b)
    assert r["n_ranges"] == nr and r["pieces"] == 2 * n and r["bytes_compared"] == size
    c = d.file("c", flipped(data, [size - 1]), tiling(la))  # the same cuts: every piece but the last shared
    r2 = d.diff(a, c)
    assert r2["ranges"] == [(size - 1, 1)] and r2["pieces"] == n and r2["bytes_compared"] == int(la[-1])
    return {"moved": r, "same_cuts": r2}


def case_insert(d, k, tables_only=False):
    """After an insert at offset 0 every later span is the same slot at a shifted
    offset: everything is compared."""
    data = rand(24, 32 << 10)
    a = d.file("a", data)
    b = d.clone("a", "b")
    d.splice(b, 0, 0, rand(2500 + k, k))
    r = d.diff(a, b, tables_only)
    assert r["bytes_shared"] == 0 and r["size_b"] == r["size_a"] + k
    assert r["bytes_compared"] == (0 if tables_only else data.size)
    if tables_only:
        assert r["ranges"] == [(0, data.size + k)]
    return {"insert": r}
