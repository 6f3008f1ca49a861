"""Python model of cdc_files_delta_device (include/chunkfs_amd.h, "Content-aligned
delta"), written for this repository over gc_model.Files, and the cases the CPU
and GPU suites share.

As in diff_model a store slot is a digest.  The model walks the rule as the
header states it, one span and one byte at a time: anchors by nearest offset,
runs, the two edges of every region, canonical form.

A case is a function of a driver and returns {label: result}.  ModelDriver runs
it on the model alone (tests/test_delta_model.py checks every result there
against the contents: rebuilt, tiled, canonical, maximal); the GPU suite's
driver runs the device layer beside the model and compares every delta.
"""
import bisect

import numpy as np

import diff_model as dm

LIT = (1 << 64) - 1
STATS = ("n_ops", "bytes_copy", "bytes_literal", "bytes_literal_tables", "spans_matched", "regions", "size_a",
         "size_b")
rand, tiling, flipped = dm.rand, dm.tiling, dm.flipped


# ---- the model ---------------------------------------------------------------------------
def anchors(sa, sb):
    """Step 1 and 2: [[first byte in B, diagonal or None]] per run, and the
    number of matched spans."""
    groups = {}
    for s in sa:
        if s.len:
            groups.setdefault(s.hash, []).append(s.offset)  # ascending: file order
    runs, matched = [], 0
    for s in sb:
        if not s.len:
            continue
        offs, d = groups.get(s.hash), None
        if offs:
            p = bisect.bisect_left(offs, s.offset)
            d = min(offs[max(p - 1, 0):p + 1], key=lambda o: (abs(o - s.offset), o)) - s.offset
            matched += 1
        if not runs or runs[-1][1] != d:
            runs.append([s.offset, d])
    return runs, matched


def canonical(ops):
    """Step 4 over (b_off, len, diagonal or None)."""
    out = []
    for b_off, ln, d in ops:
        if not ln:
            continue
        if out and d is not None and out[-1][2] == d:
            out[-1][1] += ln
        else:
            out.append([b_off, ln, d])
    return [(o, n, LIT if d is None else o + d) for o, n, d in out]


def delta(files, ha, hb, tables_only=False):
    """cdc_files_delta_device: {"ops": [(b_off, len, a_off)], and STATS}."""
    a, b = files.read_complete(ha), files.read_complete(hb)
    size_a, size_b = int(a.size), int(b.size)
    runs, matched = anchors(files._spans(ha), files._spans(hb))
    raw, regions, lit_tables = [], 0, 0
    for k, (l, d) in enumerate(runs):
        r = runs[k + 1][0] if k + 1 < len(runs) else size_b
        if d is not None:
            raw.append((l, r - l, d))
            continue
        regions += 1
        lit_tables += r - l
        e = f = 0
        dl = runs[k - 1][1] if k else 0
        dr = runs[k + 1][1] if k + 1 < len(runs) else size_a - size_b
        if not tables_only:
            while e < r - l and 0 <= l + dl + e < size_a and b[l + e] == a[l + dl + e]:
                e += 1
            while f < r - l - e and 0 <= r - 1 - f + dr < size_a and b[r - 1 - f] == a[r - 1 - f + dr]:
                f += 1
        raw += [(l, e, dl), (l + e, r - l - e - f, None), (r - f, f, dr)]
    ops = canonical(raw)
    lit = sum(n for _, n, x in ops if x == LIT)
    return {"ops": ops, "n_ops": len(ops), "bytes_copy": size_b - lit, "bytes_literal": lit,
            "bytes_literal_tables": lit_tables, "spans_matched": matched, "regions": regions, "size_a": size_a,
            "size_b": size_b}


def apply(a, ops, b):
    """B rebuilt from A, the ops and B's own bytes for the LITERALs."""
    out = np.zeros(sum(n for _, n, _ in ops), dtype=np.uint8)
    for o, n, x in ops:
        out[o:o + n] = b[o:o + n] if x == LIT else a[x:x + n]
    return out


def check(a, b, r, tables_only=False):
    """What holds for every answer, from the contents alone: the ops tile
    [0, size_b) and rebuild B, are canonical, and -- in exact mode -- no COPY
    next to a LITERAL can be extended into it."""
    ops = r["ops"]
    assert [o for o, _, _ in ops] == [0] + list(np.cumsum([n for _, n, _ in ops])[:-1]) if ops else b.size == 0
    assert sum(n for _, n, _ in ops) == b.size and all(n > 0 for _, n, _ in ops)
    assert (apply(a, ops, b) == b).all()
    assert all(x == LIT or x + n <= a.size for _, n, x in ops)
    for (o1, n1, x1), (o2, n2, x2) in zip(ops, ops[1:]):
        assert not (x1 == LIT and x2 == LIT)
        assert x1 == LIT or x2 == LIT or x1 - o1 != x2 - o2
        if tables_only:
            continue
        if x2 == LIT:  # the COPY before a LITERAL stops at a mismatch or at A's end
            assert x1 + n1 == a.size or a[x1 + n1] != b[o2]
        if x1 == LIT:  # the COPY after one starts at a mismatch or at A's start: a LITERAL is left, so f was not clipped
            assert x2 == 0 or a[x2 - 1] != b[o2 - 1]
    assert r["bytes_copy"] + r["bytes_literal"] == b.size == r["size_b"] and r["size_a"] == a.size
    assert r["bytes_literal"] <= r["bytes_literal_tables"] and r["n_ops"] == len(ops)


class ModelDriver(dm.ModelDriver):
    """diff_model's driver with the delta; every answer is checked against the contents."""

    def delta(self, a, b, tables_only=False):
        r = delta(self.m, a, b, tables_only)
        check(self.content(a), self.content(b), r, tables_only)
        return r


# ---- the cases ------------------------------------------------------------------------------
T8 = tiling([512] * 8)


def case_prototype(d):
    """The hand-cut table of the rule's first prototype, answer for answer."""
    assert d.name == "fixed"
    data = rand(51, 4096)
    a = d.file("a", data, T8)
    out = {}
    ins = np.concatenate([rand(52, 5), data])
    out["insert0"] = d.delta(a, d.file("i0", ins, tiling([512] * 8 + [5])))
    assert out["insert0"]["ops"] == [(0, 5, LIT), (5, 4096, 0)] and out["insert0"]["spans_matched"] == 0
    ow = data.copy()
    ow[1000:1003] ^= 0xFF
    b = d.file("ow", ow, T8)
    out["overwrite"] = d.delta(a, b)
    assert out["overwrite"]["ops"] == [(0, 1000, 0), (1000, 3, LIT), (1003, 3093, 1003)]
    out["overwrite_tables"] = d.delta(a, b, True)
    assert out["overwrite_tables"]["ops"] == [(0, 512, 0), (512, 512, LIT), (1024, 3072, 1024)]
    out["swapped"] = d.delta(a, d.file("sw", np.concatenate([data[2048:], data[:2048]]), T8))
    assert out["swapped"]["ops"] == [(0, 2048, 2048), (2048, 2048, 0)]
    cuts = [700, 900, 800, 600, 1096]  # CDC-like: the cut after the edit realigns
    a2 = d.file("a2", data, tiling(cuts))
    i7 = np.concatenate([data[:1200], rand(53, 7), data[1200:]])
    out["insert_mid"] = d.delta(a2, d.file("i7", i7, tiling([700, 907, 800, 600, 1096])))
    assert out["insert_mid"]["ops"] == [(0, 1200, 0), (1200, 7, LIT), (1207, 2896, 1200)]
    d100 = np.concatenate([data[:1200], data[1300:]])
    out["delete_mid"] = d.delta(a2, d.file("d100", d100, tiling([700, 800, 800, 600, 1096])))
    assert out["delete_mid"]["ops"] == [(0, 1200, 0), (1200, 2796, 1300)]
    z = d.file("z8", np.zeros(4096, np.uint8), T8)
    out["zeros"] = d.delta(z, d.file("z9", np.zeros(4608, np.uint8), tiling([512] * 9)))
    assert out["zeros"]["ops"] == [(0, 4096, 0), (4096, 512, 3584)]
    out["prefix"] = d.delta(a, d.file("pre", data[:1000], tiling([300, 700])))
    assert out["prefix"]["ops"] == [(0, 1000, 0)] and out["prefix"]["spans_matched"] == 0
    out["suffix"] = d.delta(a, d.file("suf", data[3000:], tiling([96, 1000])))
    assert out["suffix"]["ops"] == [(0, 1096, 3000)]
    e = d.file("e", data[:0])
    out["a_empty"] = d.delta(e, a)
    assert out["a_empty"]["ops"] == [(0, 4096, LIT)] and out["a_empty"]["regions"] == 1
    out["b_empty"] = d.delta(a, e)
    assert out["b_empty"]["ops"] == []
    return out


def case_insert(d, k, tables_only=False):
    """diff_model.case_insert's scenario: k bytes inserted at offset 0 of a clone."""
    data = rand(24, 32 << 10)
    a = d.file("a", data)
    b = d.clone("a", "b")
    d.splice(b, 0, 0, rand(2500 + k, k))
    r = d.delta(a, b, tables_only)
    if tables_only and d.name == "fixed":  # every cut moved: no slot survives
        assert r["ops"] == [(0, data.size + k, LIT)]
    elif tables_only:
        assert r["n_ops"] == 2 and r["ops"][0][2] == LIT and r["ops"][1][2] == r["ops"][1][0] - k
    else:
        assert r["ops"] == [(0, k, LIT), (k, data.size, 0)]
    return {"insert": r}


def case_edits(d, tables_only=False):
    """Insert, delete and overwrite in the middle of a clone, one after another."""
    data = rand(54, 96 << 10)
    a = d.file("a", data)
    b = d.clone("a", "b")
    out, mid = {}, data.size // 2 + 3
    d.splice(b, mid, 0, rand(55, 77))
    out["insert"] = d.delta(a, b, tables_only)
    d.splice(b, 9000, 300, None)
    out["delete"] = d.delta(a, b, tables_only)
    d.splice(b, 70000, 40, rand(56, 40) | 1)
    out["overwrite"] = d.delta(a, b, tables_only)
    if not tables_only:
        assert out["insert"]["ops"] == [(0, mid, 0), (mid, 77, LIT), (mid + 77, data.size - mid, mid)]
        assert out["delete"]["n_ops"] == 4 and out["delete"]["bytes_literal"] == 77
        assert out["overwrite"]["bytes_literal"] <= 77 + 40 and out["overwrite"]["n_ops"] >= 6
    else:
        assert out["overwrite"]["regions"] == 3 and out["overwrite"]["n_ops"] == 7
    out["back"] = d.delta(b, a, tables_only)
    return out


ALIGN_L = dm.ALIGN_L


def align_positions(L):
    """Where the one mismatch of a region of L bytes sits: nowhere, byte 0, the
    last byte, and either side of every 4096 tile edge counted from either end."""
    pos = {None, 0, L - 1}
    for t in range(4096, L, 4096):
        pos |= {t - 1, t, L - t - 1, L - t}
    return sorted((p for p in pos if p is not None and 0 <= p < L), key=int) + [None]


def case_alignment(d, L, k_range=range(1, 18)):
    """A = head | X | tail as three spans; B = head | X' | tail with X' cut
    [k, L - k]: the region is X', both neighbours on diagonal 0.  X' differs from
    X in one byte, or in none: then the region vanishes and the answer is one
    COPY.  Every relative misalignment of the two sides, every ragged end."""
    head, x, tail = rand(61, 100), rand(1600 + L, L), rand(62, 90)
    a = d.file(f"a{L}", np.concatenate([head, x, tail]), tiling([100, L, 90]))
    out = {}
    positions = align_positions(L)
    for n in range(max(len(k_range), len(positions))):  # every k and every position at least once
        k, p = min(k_range[n % len(k_range)], L), positions[n % len(positions)]
        xb = x if p is None else flipped(x, [p])
        cut = [100, k, L - k, 90] if k < L else [100, L, 90]
        if p is None and k == L:
            continue  # the same cuts and bytes: no region at all
        b = d.file(f"b{L}_{n}", np.concatenate([head, xb, tail]), tiling(cut))
        r = d.delta(a, b)
        want = [(0, L + 190, 0)] if p is None else [o for o in ((0, 100 + p, 0), (100 + p, 1, LIT),
                                                                   (101 + p, L + 89 - p, 101 + p)) if o[1]]
        assert r["ops"] == want, (L, p, k, r["ops"])
        assert r["regions"] == 1 and r["bytes_literal_tables"] == L
        out[f"p{p}_k{k}"] = r
    return out


def case_misalign(d, L):
    """A = P | head | X | tail with 7 bytes P, B = head | X' | tail with X' cut
    [k, L - k] for every k = 1..17: both neighbours on diagonal 7, so A's side of
    the region is 7 + k bytes off B's whatever the arena gives.  X' differs in
    two bytes, the first and the last found by different blocks once L spans
    tiles."""
    head, x, tail = rand(63, 64), rand(1700 + L, L), rand(64, 80)
    a = d.file(f"a{L}", np.concatenate([rand(65, 7), head, x, tail]), tiling([7, 64, L, 80]))
    out = {}
    lo, hi = min(2, L - 1), max(L - 3, 0)
    lo, hi = min(lo, hi), max(lo, hi)
    xb = flipped(x, sorted({lo, hi}))
    for k in range(1, 18):
        if k > L:
            break
        b = d.file(f"b{L}_{k}", np.concatenate([head, xb, tail]), tiling([64, k, L - k, 80] if k < L else [64, L, 80]))
        r = d.delta(a, b)
        assert r["ops"] == [(0, 64 + lo, 7), (64 + lo, hi - lo + 1, LIT), (65 + hi, L + 79 - hi, 72 + hi)], (L, k)
        assert r["regions"] == 1 and r["bytes_literal_tables"] == L
        out[f"k{k}"] = r
    return out


def case_overlap(d):
    """Forward takes precedence; the searches stop at A's ends."""
    z = np.zeros(512, np.uint8)
    out = {}
    # zeros between zero neighbours: A = Z Z, B = Z z' Z with z' 300 zeros cut as its own slot
    a = d.file("a", np.concatenate([z, z]), tiling([512, 512]))
    b = d.file("b", np.zeros(1324, np.uint8), tiling([512, 300, 512]))
    out["zeros"] = d.delta(a, b)
    assert out["zeros"]["regions"] == 1 and out["zeros"]["bytes_literal"] == 0
    # forward cut short by size_a: B goes on past A's end with A's last bytes again
    x = rand(71, 600)
    a2 = d.file("a2", x, tiling([600]))
    b2 = d.file("b2", np.concatenate([x, x[-50:], rand(72, 10)]), tiling([600, 60]))
    out["past_end"] = d.delta(a2, b2)
    assert out["past_end"]["ops"] == [(0, 600, 0), (600, 60, LIT)]
    # backward cut short by A's offset 0
    b3 = d.file("b3", np.concatenate([rand(73, 10), x[:50], x]), tiling([60, 600]))
    out["before_start"] = d.delta(a2, b3)
    assert out["before_start"]["ops"] == [(0, 60, LIT), (60, 600, 0)]
    # both directions meet: B = A with its middle span cut in two, equal bytes -- forward takes all
    y = rand(74, 900)
    a4 = d.file("a4", y, tiling([300, 300, 300]))
    out["meet"] = d.delta(a4, d.file("b4", y, tiling([300, 100, 200, 300])))
    assert out["meet"]["ops"] == [(0, 900, 0)]
    return out


def case_nearest(d):
    X, Y = rand(81, 256), rand(82, 256)
    out = {}
    # a tie: B's X at 256 lies between A's X at 0 and at 512; the smaller offset wins
    a = d.file("xyx", np.concatenate([X, Y, X]), tiling([256] * 3))
    out["tie"] = d.delta(a, d.file("yxy", np.concatenate([Y, X, Y]), tiling([256] * 3)))
    assert out["tie"]["ops"] == [(0, 256, 256), (256, 512, 0)]  # the larger would give (256, 256, 512) and a third op
    out["xyx_xxy"] = d.delta(a, d.file("xxy", np.concatenate([X, X, Y]), tiling([256] * 3)))
    assert out["xyx_xxy"]["ops"] == [(0, 256, 0), (256, 512, 0)]  # the second X ties too and goes back to A's first
    # zero runs against longer and shorter ones
    z = lambda n: np.zeros(64 * n, np.uint8)  # noqa: E731
    z10 = d.file("z10", z(10), tiling([64] * 10))
    out["longer"] = d.delta(z10, d.file("z13", z(13), tiling([64] * 13)))
    assert out["longer"]["ops"] == [(0, 640, 0), (640, 64, 576), (704, 64, 576), (768, 64, 576)]  # A's last, thrice
    out["shorter"] = d.delta(z10, d.file("z4", z(4), tiling([64] * 4)))
    assert out["shorter"]["ops"] == [(0, 256, 0)]
    # a slot group of 2049 equal spans: past one scan block
    n = 2049
    big = d.file("big", np.zeros(16 * n, np.uint8), tiling([16] * n))
    out["group"] = d.delta(big, d.file("big2", np.concatenate([rand(83, 16) | 1, np.zeros(16 * n, np.uint8)]),
                                       tiling([16] * (n + 1))))
    assert out["group"]["ops"] == [(0, 16, LIT), (16, 16 * (n - 1), 16), (16 * n, 16, 16 * (n - 1))]
    data = rand(84, 4096)
    h = d.file("h", data, T8)
    out["swapped"] = d.delta(h, d.file("hs", np.concatenate([data[2048:], data[:2048]]), T8))
    assert out["swapped"]["ops"] == [(0, 2048, 2048), (2048, 2048, 0)]
    return out


def case_empty_spans(d):
    """Spans of length 0 in both tables: at the start, between runs, inside a
    region, at the end."""
    data = rand(91, 600)
    a = d.file("a", data, [[0, 0], [0, 200], [200, 0], [200, 0], [200, 200], [400, 200], [600, 0]])
    nb = flipped(data, [250])
    b = d.file("b", nb, [[0, 0], [0, 0], [0, 200], [200, 0], [200, 100], [300, 0], [300, 100], [400, 0], [400, 200],
                         [600, 0]])
    r = d.delta(a, b)
    assert r["ops"] == [(0, 250, 0), (250, 1, LIT), (251, 349, 251)] and r["spans_matched"] == 2
    r2 = d.delta(b, a)
    assert r2["ops"] == [(0, 250, 0), (250, 1, LIT), (251, 349, 251)]
    return {"ab": r, "ba": r2, "tables": d.delta(a, b, True)}


def case_degenerate(d):
    data = rand(92, 3000)
    a = d.file("a", data, tiling([1000] * 3))
    e1, e2 = d.file("e1", data[:0]), d.file("e2", data[:0])
    z = d.file("z", data[:0], [[0, 0], [0, 0]])  # spans, and no byte
    out = {"a_e": d.delta(a, e1), "e_a": d.delta(e1, a), "e_e": d.delta(e1, e2), "z_a": d.delta(z, a),
           "a_z": d.delta(a, z), "e_z": d.delta(e1, z), "self": d.delta(a, a), "self_e": d.delta(e1, e1),
           "e_a_tables": d.delta(e1, a, True)}
    assert out["e_a"]["ops"] == out["z_a"]["ops"] == out["e_a_tables"]["ops"] == [(0, 3000, LIT)]
    assert out["a_e"]["ops"] == out["e_e"]["ops"] == out["a_z"]["ops"] == out["self_e"]["ops"] == []
    assert out["self"]["ops"] == [(0, 3000, 0)] and out["self"]["spans_matched"] == 3
    # no slot in common: the prefix and suffix rule, equal and unequal sizes
    other = data.copy()
    other[1400:1600] ^= 0x3C
    out["equal_sizes"] = d.delta(a, d.file("o", other, tiling([750] * 4)))
    assert out["equal_sizes"]["ops"] == [(0, 1400, 0), (1400, 200, LIT), (1600, 1400, 1600)]
    grown = np.concatenate([data[:1400], rand(93, 333), data[1400:]])
    out["unequal_sizes"] = d.delta(a, d.file("g", grown, tiling([1111] * 3)))
    assert out["unequal_sizes"]["ops"] == [(0, 1400, 0), (1400, 333, LIT), (1733, 1600, 1400)]
    out["nothing_shared"] = d.delta(a, d.file("n", ~data, tiling([1500] * 2)))
    assert out["nothing_shared"]["ops"] == [(0, 3000, LIT)]
    out["tables"] = d.delta(a, d.file("g2", grown, tiling([1111, 2222])), True)
    assert out["tables"]["ops"] == [(0, 3333, LIT)]
    return out


# (changed spans = regions, does a kept span lead) -> ops: 2047, 2048 and 2049 of either
COUNT_CASES = {(1023, True): 2047, (1024, False): 2048, (1024, True): 2049, (2047, True): 4095, (2048, False): 4096,
               (2049, True): 4099}


def case_counts(d, changed, lead):
    """Alternating kept and changed spans of 16 - 64 bytes: `changed` regions,
    every one differing in its middle byte alone.  Each gives three ops whose
    COPYs join the kept spans.  Without a kept span in front the file's first
    byte differs, so the script opens with a LITERAL and has an even length."""
    rng = np.random.default_rng(3100 + changed)
    n = 2 * changed + (1 if lead else 0)
    la = rng.integers(16, 65, n)
    off = np.concatenate([[0], np.cumsum(la)])
    data = rand(3200 + changed, int(la.sum()))
    first = 1 if lead else 0
    mids = [int(off[i] + la[i] // 2) for i in range(first, n, 2)]
    if not lead:
        mids[0] = 0
    a = d.file("a", data, tiling(la))
    b = d.file("b", flipped(data, mids), tiling(la))
    r = d.delta(a, b)
    assert r["regions"] == changed and r["n_ops"] == COUNT_CASES[changed, lead] and r["bytes_literal"] == changed
    rt = d.delta(a, b, True)
    assert rt["regions"] == changed and rt["n_ops"] == 2 * changed + (1 if lead else 0)
    return {"exact": r, "tables": rt}
