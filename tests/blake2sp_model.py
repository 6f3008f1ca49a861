"""BLAKE2sp-256, unkeyed: the oracle and a from-scratch twin of the device kernel
(chunkfs_amd/csrc/blake2sp.hip, DESIGN.md "Hashers").

The oracle is hashlib.blake2s with the tree parameters: 8 leaves that take the
message's 64-byte blocks round-robin, and a root over the 8 leaf digests.  It is
exact and fast; the GPU tests compare with it.

The twin is written the way the kernel is, so that a kernel bug can be chased on
the CPU: a chunk is a GROUP of 8 lanes, lane g is leaf g, step j gives lane g
block 8j + g, the lanes of all groups run one compression per step in lockstep
(numpy arrays with one column per lane), lanes without a block are masked, the
byte counter and the finalisation flags are per lane, and after its last leaf
step a group spends four steps on the root in lane 0, whose message words are
the leaf digests of its neighbours.  compress_int is the same compression on
plain Python integers, one lane at a time.
"""
import hashlib

import numpy as np

IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
SIGMA = (
    (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15), (14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3),
    (11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4), (7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8),
    (9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13), (2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9),
    (12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11), (13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10),
    (6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5), (10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0))

# Parameter block (RFC 7693 2.5), as the four words that are not zero or the
# node offset: digest length 32, no key, fanout 8, depth 2 | inner length 32
# with node depth 0 (leaf) or 1 (root).
PARAM0 = 32 | (0 << 8) | (8 << 16) | (2 << 24)
PARAM3_LEAF = (0 << 16) | (32 << 24)
PARAM3_ROOT = (1 << 16) | (32 << 24)

KNOWN = {
    b"": "dd0e891776933f43c7d032b08a917e25741f8aa9a12c12e1cac8801500f2ca4f",  # the published BLAKE2sp answer
    b"\x00": "a6b9eecc25227ad788c99d3f236debc8da408849e9a5178978727a81457f7239",
    bytes(range(255)): "25059f10605e67adfe681350666e15ae976a5a571c13cf5bc8053f430e120a52",
}

M32 = 0xFFFFFFFF


# ---- the oracle ---------------------------------------------------------------------
def oracle(d):
    d = bytes(d)
    leaves = [b"".join(d[o:o + 64] for o in range(64 * i, len(d), 512)) for i in range(8)]
    kw = dict(digest_size=32, fanout=8, depth=2, leaf_size=0, inner_size=32)
    mid = b"".join(hashlib.blake2s(leaves[i], node_offset=i, node_depth=0, last_node=(i == 7), **kw).digest()
                   for i in range(8))
    return hashlib.blake2s(mid, node_offset=0, node_depth=1, last_node=True, **kw).digest()


def digests(buf, chunks):
    """(n, 32) uint8: the oracle over buf[offset : offset + length] of every chunk."""
    b = bytes(buf)
    out = np.zeros((len(chunks), 32), dtype=np.uint8)
    for i, (o, n) in enumerate(chunks):
        out[i] = np.frombuffer(oracle(b[int(o):int(o) + int(n)]), dtype=np.uint8)
    return out


# ---- the twin -----------------------------------------------------------------------
def param_words(node_offset, root):
    """h at the start of a node: IV ^ parameter block."""
    h = list(IV)
    h[0] ^= PARAM0
    h[2] ^= node_offset & M32
    h[3] ^= ((node_offset >> 32) & 0xFFFF) | (PARAM3_ROOT if root else PARAM3_LEAF)
    return h


def _rotr_int(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def compress_int(h, m, t, f0, f1):
    """One compression on Python integers: h (8 words), m (16 words), the 64-bit
    byte counter t, the flag words f0 / f1.  Returns the new h."""
    v = list(h) + list(IV)
    v[12] ^= t & M32
    v[13] ^= (t >> 32) & M32
    v[14] ^= f0
    v[15] ^= f1

    def g(a, b, c, d, x, y):
        v[a] = (v[a] + v[b] + x) & M32
        v[d] = _rotr_int(v[d] ^ v[a], 16)
        v[c] = (v[c] + v[d]) & M32
        v[b] = _rotr_int(v[b] ^ v[c], 12)
        v[a] = (v[a] + v[b] + y) & M32
        v[d] = _rotr_int(v[d] ^ v[a], 8)
        v[c] = (v[c] + v[d]) & M32
        v[b] = _rotr_int(v[b] ^ v[c], 7)

    for r in range(10):
        s = SIGMA[r]
        g(0, 4, 8, 12, m[s[0]], m[s[1]])
        g(1, 5, 9, 13, m[s[2]], m[s[3]])
        g(2, 6, 10, 14, m[s[4]], m[s[5]])
        g(3, 7, 11, 15, m[s[6]], m[s[7]])
        g(0, 5, 10, 15, m[s[8]], m[s[9]])
        g(1, 6, 11, 12, m[s[10]], m[s[11]])
        g(2, 7, 8, 13, m[s[12]], m[s[13]])
        g(3, 4, 9, 14, m[s[14]], m[s[15]])
    return [h[i] ^ v[i] ^ v[i + 8] for i in range(8)]


_SX = [np.array(s[0:8:2]) for s in SIGMA], [np.array(s[1:8:2]) for s in SIGMA]
_SD = [np.array(s[8:16:2]) for s in SIGMA], [np.array(s[9:16:2]) for s in SIGMA]


_ROT = [np.array([(i + k) % 4 for i in range(4)]) for k in range(4)]


_SH = {n: (np.uint32(n), np.uint32(32 - n)) for n in (16, 12, 8, 7)}


def _xor_rotr(x, y, n):
    """rotr(x ^ y, n), into x."""
    np.bitwise_xor(x, y, out=x)
    hi = np.left_shift(x, _SH[n][1])
    np.right_shift(x, _SH[n][0], out=x)
    np.bitwise_or(x, hi, out=x)


def _g4(a, b, c, d, x, y):
    """G on four (a, b, c, d) at once, in place."""
    a += b
    a += x
    _xor_rotr(d, a, 16)
    c += d
    _xor_rotr(b, c, 12)
    a += b
    a += y
    _xor_rotr(d, a, 8)
    c += d
    _xor_rotr(b, c, 7)


def compress(h, m, t, f0, f1):
    """One compression in every lane: h (8, L), m (16, L) uint32, t (L,) uint64,
    f0 / f1 (L,) uint32.  Returns the new h; the four G of a half round run
    together (the rows of a, b, c, d), the lanes as columns."""
    lanes = h.shape[1]
    a, b = h[0:4].copy(), h[4:8].copy()
    c = np.repeat(np.array(IV[0:4], dtype=np.uint32)[:, None], lanes, axis=1)
    d = np.repeat(np.array(IV[4:8], dtype=np.uint32)[:, None], lanes, axis=1)
    d[0] ^= (t & np.uint64(M32)).astype(np.uint32)
    d[1] ^= (t >> np.uint64(32)).astype(np.uint32)
    d[2] ^= f0
    d[3] ^= f1
    for r in range(10):
        _g4(a, b, c, d, m[_SX[0][r]], m[_SX[1][r]])
        b, c, d = b[_ROT[1]], c[_ROT[2]], d[_ROT[3]]  # the diagonals: row i takes b[i+1], c[i+2], d[i+3]
        _g4(a, b, c, d, m[_SD[0][r]], m[_SD[1][r]])
        b, c, d = b[_ROT[3]], c[_ROT[2]], d[_ROT[1]]
    return h ^ np.concatenate([a, b]) ^ np.concatenate([c, d])


def _blocks(data, step):
    """The 8 message blocks of a group's step, (16, 8) words: lane g gets the 64
    bytes at 64 * (8 * step + g), zero-filled from the chunk's end on."""
    part = data[512 * step:512 * step + 512]
    if len(part) < 512:
        part = part + bytes(512 - len(part))
    return np.frombuffer(part, dtype="<u4").reshape(8, 16).T


def blake2sp_many(chunks):
    """The digests of `chunks` (byte strings), one group of 8 lanes each, all
    groups stepping together as the groups of a wave do."""
    chunks = [bytes(c) for c in chunks]
    n = len(chunks)
    if n == 0:
        return []
    lens = np.array([len(c) for c in chunks], dtype=np.uint64)
    nb = (lens + np.uint64(63)) // np.uint64(64)
    nsteps = np.maximum((nb + np.uint64(7)) // np.uint64(8), np.uint64(1))  # (an empty chunk finalises 8 empty leaves)
    lanes = 8 * n
    g = np.tile(np.arange(8, dtype=np.uint64), n)
    grp = np.repeat(np.arange(n), 8)
    L_len, L_nb, L_nsteps = lens[grp], nb[grp], nsteps[grp]
    h = np.zeros((8, lanes), dtype=np.uint32)
    dg = np.zeros((8, lanes), dtype=np.uint32)
    out = [None] * n
    leaf0 = np.array([param_words(i, False) for i in range(8)], dtype=np.uint32).T  # (8 words, 8 leaves)
    root0 = np.array(param_words(0, True), dtype=np.uint32)
    for step in range(int(nsteps.max()) + 4):
        s = np.uint64(step)
        have = s < L_nsteps + np.uint64(4)
        root = have & (s >= L_nsteps)
        rb = np.where(root, s - L_nsteps, 0).astype(np.int64)
        k = np.uint64(8) * s + g
        leaf = have & ~root & ((k < L_nb) | (step == 0))
        if step == 0:
            h = np.tile(leaf0, (1, n))
        first_root = root & (rb == 0)
        h[:, first_root] = root0[:, None]
        m = np.zeros((16, lanes), dtype=np.uint32)
        for c in range(n):
            if step < int(nsteps[c]):
                m[:, 8 * c:8 * c + 8] = _blocks(chunks[c], step)
            elif step < int(nsteps[c]) + 4:
                r = step - int(nsteps[c])  # root block r = the digests of leaves 2r and 2r + 1, in lane 0
                m[:, 8 * c] = np.concatenate([dg[:, 8 * c + 2 * r], dg[:, 8 * c + 2 * r + 1]])
        in_chunk = k < L_nb
        rest = np.where(in_chunk, L_len - np.uint64(64) * np.where(in_chunk, k, 0), 0).astype(np.uint64)
        t_leaf = np.where(in_chunk, np.uint64(64) * s + np.minimum(rest, np.uint64(64)), 0).astype(np.uint64)
        t = np.where(root, np.uint64(64) * (rb.astype(np.uint64) + np.uint64(1)), t_leaf).astype(np.uint64)
        fin = np.where(root, rb == 3, k + np.uint64(8) >= L_nb)
        f0 = np.where(fin, M32, 0).astype(np.uint32)
        f1 = np.where(fin & (root | (g == 7)), M32, 0).astype(np.uint32)
        act = leaf | (root & (g == 0))
        hn = compress(h, m, t, f0, f1)
        h = np.where(act[None, :], hn, h)
        dg = np.where((leaf & fin)[None, :], hn, dg)
        for c in np.nonzero(root[::8] & (rb[::8] == 3))[0]:
            out[c] = h[:, 8 * c].astype("<u4").tobytes()
    return out


def blake2sp(data):
    return blake2sp_many([data])[0]


for _d, _hex in KNOWN.items():
    assert oracle(_d).hex() == _hex, _hex
