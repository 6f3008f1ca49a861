"""Python model of cdc_file_splice_device (include/chunkfs_amd.h, "Editing a file
in place"), written for this repository: the rule in plain Python over
files_model.Files and store_model.Model, chunking with the oracle (oracle.py) or
ae_model.py, and the cases the CPU and GPU suites share.

splice() follows the header's four steps.  windowed=True chunks the windows the
engine chunks (every round from off[i0] again) and reports rounds and
window_bytes; windowed=False chunks the whole tail as one buffer.  The two must
agree (tests/test_splice_model.py).
"""
import bisect

import numpy as np

import ae_model
import files_model as fm
import oracle

BACK = 8  # bytes a rule may read at or past its cut (AE: the bytes i .. i+3 of the cut after byte i)

# name -> (algorithm, min, avg, max); "fixed": the chunk size
CHUNKERS = {"fast": ("fast", 64, 256, 1024), "rabin": ("rabin", 64, 256, 1024), "ultra": ("ultra", 64, 256, 1024),
            "leap": ("leap", 64, 256, 1024), "seq": ("seq", 64, 256, 1024), "ae": ("ae", 64, 256, 1024),
            "fixed": ("fixed", 512, 0, 0)}
CDC = [k for k in CHUNKERS if k != "fixed"]


def max_chunk(name):
    algo, mn, _, mx = CHUNKERS[name]
    return mn if algo == "fixed" else mx


def chunk(name, data):
    """chunk_data of the named chunker over one buffer: (n, 2) uint64 offset / length."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if data.size == 0:
        return np.zeros((0, 2), dtype=np.uint64)
    algo, mn, avg, mx = CHUNKERS[name]
    if algo == "fixed":
        return oracle.fixed(data.size, mn)
    if algo == "fast":
        return oracle.fastcdc(data, mn, avg, mx)
    if algo == "ae":
        return ae_model.chunk_array(data, mn, avg, mx)
    return oracle.cdc(algo, data, mn, avg, mx)


def make_chunker(c, name):
    """The device chunker of the same name and sizes."""
    algo, mn, avg, mx = CHUNKERS[name]
    if algo == "fixed":
        return c.FSChunker(mn)
    sizes = c.SizeParams(mn, avg, mx)
    if algo == "seq":
        return c.SeqChunker(c.OperationMode.Increasing, sizes)
    if algo == "ae":
        return c.AeChunker(sizes)
    return {"fast": c.FastChunker, "rabin": c.RabinChunker, "ultra": c.UltraChunker, "leap": c.LeapChunker}[algo](sizes)


def window_end(size_after, offset, insert_len, mx, rnd):
    return min(size_after, offset + insert_len + 4 ** rnd * mx + BACK)


def start_span(offs, n, offset):
    """Step 1: the last span with off + 8 <= offset, among equal offsets the last; 0 if none."""
    i0 = 0
    for i in range(n):
        if offs[i] + BACK <= offset:
            i0 = i
    return i0


def splice(files, h, name, offset, remove_len, ins, windowed=True):
    """The rule on the model's file; returns the stats dict (cdc_splice_stats_t's
    fields; window_bytes is the restart-from-off[i0] figure; both 0 when
    windowed=False).  Refusals are the caller's to model."""
    spans = files._spans(h)
    ins = np.ascontiguousarray(ins if ins is not None else np.zeros(0, np.uint8), dtype=np.uint8)
    old = files.read_complete(h)
    n, size = len(spans), old.size
    assert offset <= size and offset + remove_len <= size
    if remove_len == 0 and ins.size == 0:
        return None
    new = np.concatenate([old[:offset], ins, old[offset + remove_len:]])
    delta, lo, mx = ins.size - remove_len, offset + ins.size, max_chunk(name)
    offs = [sp.offset for sp in spans] + [size]
    i0 = start_span(offs, n, offset)
    w0 = offs[i0] if n else 0

    def meet(win_end):
        """The accepted chunks of the window [w0, win_end): (chunks, j) or None."""
        cuts = chunk(name, new[w0:win_end])
        for k, (o, ln) in enumerate(cuts):
            s, e = w0 + int(o), w0 + int(o) + int(ln)
            if not (win_end == new.size or s + mx + BACK <= win_end):
                return None  # the trusted chunks are a prefix
            if e < lo:
                continue
            j = bisect.bisect_left(offs, e - delta)
            if j <= n and offs[j] == e - delta:
                return cuts[:k + 1], j
        return None

    rounds, window_bytes, got = 1, 0, None
    if new.size > w0:
        if windowed:
            rounds = 0
            while got is None:
                rounds += 1
                end_w = window_end(new.size, offset, ins.size, mx, rounds)
                window_bytes += end_w - w0
                got = meet(end_w)
                assert got is not None or end_w < new.size, "a window that ends with the file always resyncs"
        else:
            got = meet(new.size)
            rounds = 0
    accepted, j = got if got is not None else (np.zeros((0, 2), np.uint64), n)
    before = files.store.stats()["unique_bytes"]
    dig, _ = files.store.put(new[w0:], accepted) if len(accepted) else ([], None)
    bytes_new = files.store.stats()["unique_bytes"] - before
    fresh = [fm.Span(bytes(d), w0 + int(o), int(ln)) for d, (o, ln) in zip(dig, accepted)]
    tail = [fm.Span(sp.hash, sp.offset + delta, sp.len) for sp in spans[j:]]
    e_k = fresh[-1].offset + fresh[-1].len if fresh else new.size
    files.files[h.name] = spans[:i0] + fresh + tail
    return {"first_span": i0, "spans_removed": j - i0, "spans_inserted": len(fresh), "resync_offset": e_k,
            "size_before": size, "size_after": new.size, "bytes_new": bytes_new, "window_bytes": window_bytes,
            "rounds": rounds}


def table(files, h):
    """[(offset, length, digest)] of the file."""
    return [(sp.offset, sp.len, sp.hash) for sp in files._spans(h)]


def twin(name, content):
    """The table a single write of `content` with the chunker makes."""
    f = fm.Files()
    h = f.create("twin")
    f.append(h, content, chunk(name, content))
    return table(f, h)


# ---- data and cases ------------------------------------------------------------------------
def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


_BASE = {}


def base(name, seed=1, n=256 << 10):
    """(data, chunks) of the n random bytes every per-chunker case starts from."""
    key = (name, seed, n)
    if key not in _BASE:
        data = rand(seed, n)
        _BASE[key] = (data, chunk(name, data))
    return _BASE[key]


EDITS = [("overwrite", 1), ("overwrite", 100), ("overwrite", 5000), ("insert", 1), ("insert", 777),
         ("delete", 1), ("delete", 3000)]
PLACES = ["first", "middle", "last"]


def place(chunks, size, kind, length, where):
    """(offset, remove_len, insert_len) of an edit of `length` bytes that starts in
    the first span, starts in the middle span, or ends inside the last span."""
    o_last, l_last = int(chunks[-1][0]), int(chunks[-1][1])
    if where == "first":
        offset = int(chunks[0][1]) // 2
    elif where == "middle":
        o, ln = chunks[len(chunks) // 2]
        offset = int(o) + int(ln) // 2
    elif kind == "insert":
        offset = o_last + l_last // 2
    else:
        offset = size - length - (1 if l_last >= 2 else 0)  # its last byte is one of the last span's
    remove_len = 0 if kind == "insert" else length
    insert_len = 0 if kind == "delete" else length
    return offset, remove_len, insert_len


def random_cases(name):
    """The 21 (label, offset, remove_len, inserted bytes) edits of the named chunker's base file."""
    _, chunks = base(name)
    out = []
    for k, (kind, length) in enumerate(EDITS):
        for w, where in enumerate(PLACES):
            offset, rem, ins = place(chunks, 256 << 10, kind, length, where)
            out.append((f"{kind}{length}_{where}", offset, rem, rand(1000 + 10 * k + w, ins)))
    return out


def exact_block(name, old, seed=77):
    """Bytes that, put in front of `old`, are chunked into whole chunks of their
    own: a cut falls exactly behind their last byte.  A rule may read a few bytes
    at or past its cut (FastCDC's hash takes in the byte at the cut), so the block
    is found by trying prefixes of a random buffer in front of `old`."""
    buf, head = rand(seed, 8 << 10), old[:4 * max_chunk(name)]
    for length in range(2 * max_chunk(name) + 1, buf.size):
        cuts = chunk(name, np.concatenate([buf[:length], head]))
        if length in (cuts[:, 0] + cuts[:, 1]).tolist():
            return buf[:length]
    raise AssertionError("no prefix ends on a cut")


def edge_cases(name="fast"):
    """label -> (offset, remove_len, inserted bytes) on the named chunker's base
    file; test_splice_model.py asserts that each lands where its name says."""
    data, chunks = base(name)
    size, mid = data.size, len(chunks) // 2
    b = int(chunks[mid][0])
    return {
        "at_boundary": (b, 0, rand(2001, 5)),
        "boundary_plus_7": (b + 7, 0, rand(2002, 5)),
        "boundary_plus_8": (b + 8, 0, rand(2003, 5)),
        "near_zero": (3, 2, rand(2004, 9)),
        "append": (size, 0, rand(2005, 300)),
        "truncate_to_0": (0, size, None),
        "truncate_to_1": (1, size - 1, None),
        "truncate_to_boundary": (b, size - b, None),
        "delete_all": (0, size, None),
        "exact_block_at_0": (0, 0, exact_block(name, data)),
    }


def round_cases():
    """label -> (chunker, file content, offset, remove_len, inserted bytes): edits
    whose cuts never meet the old ones before the end of the file, and one that
    meets them at once."""
    return {
        "zeros_fast_insert_1": ("fast", np.zeros(64 << 10, np.uint8), 100, 0, np.zeros(1, np.uint8)),
        "fixed_insert_1": ("fixed", rand(3001, 64 << 10), 20000, 0, rand(3002, 1)),
        "fixed_insert_512": ("fixed", rand(3001, 64 << 10), 40 * 512, 0, rand(3003, 512)),
    }


def random_script(seed, size, steps=20):
    """`steps` edits (offset, remove_len, insert_len) of a file that starts at
    `size` bytes, each valid for the size the ones before it leave."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        kind = rng.integers(0, 4)
        offset = int(rng.integers(0, size + 1))
        rem = 0 if kind == 1 else int(min(size - offset, rng.integers(1, 6000)))
        ins = 0 if kind == 2 else int(rng.integers(1, 6000))
        if kind == 0:
            ins = rem = min(rem, ins)
        if rem == 0 and ins == 0:
            ins = 1
        out.append((offset, rem, ins))
        size += ins - rem
    return out
