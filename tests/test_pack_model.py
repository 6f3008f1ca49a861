"""CPU suite of the pack model (tests/pack_model.py): the model must itself keep
the contract the GPU suite holds the engine to -- a full pack unpacked into an
empty store is the file written in one call; an incremental pack plus the base
is the full file; and every shared corruption is refused by the check it is
listed under, and by no earlier one."""
import struct

import numpy as np
import pytest

import diff_model as dm
import gc_model as gm
import pack_model as pm
import splice_model as spm


def written(name, data, chunks, files=None):
    """A model layer with the file written in one call."""
    files = files if files is not None else gm.Files()
    h = files.create(name)
    if len(chunks):
        files.append(h, data, chunks)
    return files, h


def same_file(fa, ha, fb, hb):
    a, b = fa._spans(ha), fb._spans(hb)
    assert [(s.hash, s.offset, s.len) for s in a] == [(s.hash, s.offset, s.len) for s in b]
    assert (fa.read_complete(ha) == fb.read_complete(hb)).all()


def same_store(fa, fb):
    assert list(fa.store.db.items()) == list(fb.store.db.items())  # the order is the arena's
    assert fa.store.stats() == fb.store.stats()


def cases():
    out = dict(pm.shapes())
    for name, seed, size in (("fast", 11, 40000), ("fixed", 12, 20 * 512 + 77)):
        data = pm.rand(seed, size)
        out["chunker " + name] = (data, spm.chunk(name, data))
    return out


CASES = cases()


@pytest.mark.parametrize("label", list(CASES))
def test_a_full_pack_unpacked_into_an_empty_store_is_the_file_written_in_one_call(label):
    data, chunks = CASES[label]
    src, h = written("f", data, chunks)
    blob, st = pm.pack(src, h)
    assert len(blob) == st["pack_bytes"] and len(blob) % 16 == 0
    assert st["spans"] == len(chunks) and st["external_spans"] == 0 and st["file_size"] == int(chunks[:, 1].sum())
    assert st["chunks"] == len({s.hash for s in src._spans(h)})
    dst = gm.Files()
    got = pm.unpack(dst, "f", blob)
    assert got == dict(st, chunks_new=st["chunks"])
    same_file(src, h, dst, dst.open("f"))
    same_store(src, dst)
    assert pm.pack(dst, dst.open("f"))[0] == blob  # deterministic, and a fixed point


def test_the_format_by_hand():
    data, chunks = CASES["padding lengths"]
    src, h = written("f", data, chunks)
    blob, _ = pm.pack(src, h)
    n, lengths = 5, [1, 15, 16, 17, 33]
    assert blob[:8] == b"CDCPACK1" and struct.unpack_from("<II", blob, 8) == (1, 0)
    size, spans, nc, ext, data_bytes, total = struct.unpack_from("<6Q", blob, 16)
    assert (size, spans, nc, ext, data_bytes, total) == (82, n, n, 0, 16 + 16 + 16 + 32 + 48, len(blob))
    at = 64 + 32 * n
    assert struct.unpack_from("<5Q", blob, at) == tuple(lengths) and blob[at + 40:at + 48] == bytes(8)
    at += 48
    assert struct.unpack_from("<5Q", blob, at) == (0, 1, 2, 3, 4)
    at += 48
    assert struct.unpack_from("<5Q", blob, at) == (0, 1, 2, 3, 4)
    at += 48
    assert struct.unpack_from("<6Q", blob, at) == (0, 16, 32, 48, 80, 128)
    at += 48
    assert len(blob) == at + 128
    off = 0
    for ln, o in zip(lengths, (0, 16, 32, 48, 80)):
        assert blob[at + o:at + o + ln] == data[off:off + ln].tobytes()
        assert blob[at + o + ln:at + o + pm.pad16(ln)] == bytes(pm.pad16(ln) - ln)  # every padding byte is zero
        off += ln
    empty, _ = pm.pack(*written("e", *CASES["empty"]))
    assert len(empty) == 64 and struct.unpack_from("<6Q", empty, 16) == (0, 0, 0, 0, 0, 64)


def edited():
    """A base, a clone of it, and the clone after one overwrite and one insert."""
    data = pm.rand(21, 48 << 10)
    src, h = written("a", data, spm.chunk("fast", data))
    dm.clone(src, "a", "base")
    spm.splice(src, h, "fast", 20000, 1024, pm.rand(22, 1024))
    spm.splice(src, h, "fast", 5000, 0, pm.rand(23, 300))
    return src, h, src.open("base")


def test_an_incremental_pack_plus_the_base_is_the_full_file():
    src, h, base = edited()
    full, _ = pm.pack(src, h)
    inc, st = pm.pack(src, h, since=base)
    old = {s.hash for s in src._spans(base)}
    new = []
    for s in src._spans(h):
        if s.hash not in old and s.hash not in new:
            new.append(s.hash)
    assert st["chunks"] == len(new) > 0 and st["external_spans"] == sum(s.hash in old for s in src._spans(h)) > 0
    assert len(inc) < len(full)
    # the receiver got the base through a full pack
    dst = gm.Files()
    pm.unpack(dst, "base", pm.pack(src, base)[0])
    # `have` from the receiver's contains is the same pack when it holds exactly the base
    have = [dst.store.contains(s.hash) for s in src._spans(h)]
    assert pm.pack(src, h, have=have)[0] == inc
    got = pm.unpack(dst, "a", inc)
    assert got["chunks_new"] == st["chunks"] and got["external_spans"] == st["external_spans"]
    same_file(src, h, dst, dst.open("a"))
    # since == the file itself carries nothing
    none, st0 = pm.pack(src, h, since=h)
    assert st0["chunks"] == 0 and st0["external_spans"] == st0["spans"] and st0["chunk_bytes"] == 0
    # without the base the externals are missing, and nothing changed
    bare = gm.Files()
    with pytest.raises(pm.PackError) as e:
        pm.unpack(bare, "a", inc)
    assert e.value.code == pm.ENOTFOUND and bare.files == {} and bare.store.db == {}


def test_refusals_of_the_model_change_nothing():
    data, chunks = pm.corrupt_source()
    src, h = written("f", data, chunks)
    blob, st = pm.pack(src, h)
    dst = gm.Files()
    pm.unpack(dst, "f", blob)
    before = (dst.store.stats(), dst.list())
    with pytest.raises(pm.PackError) as e:
        pm.unpack(dst, "f", blob)
    assert e.value.code == pm.EEXIST and (dst.store.stats(), dst.list()) == before
    arena = sum(pm.pad16(int(ln)) for ln in (100, 32, 17, 1))
    for kw in ({"arena": arena - 16}, {"max_chunks": st["chunks"] - 1}):
        small = gm.Files()
        with pytest.raises(pm.PackError) as e:
            pm.unpack(small, "f", blob, **kw)
        assert e.value.code == pm.ENOMEM and small.files == {} and small.store.db == {}
    assert pm.unpack(gm.Files(), "f", blob, arena=arena, max_chunks=st["chunks"])["chunks_new"] == 4


def test_each_corruption_is_refused_by_its_check_and_no_earlier_one():
    data, chunks = pm.corrupt_source()
    src, h = written("f", data, chunks)
    good, _ = pm.pack(src, h)
    seen = set()
    for label, blob, length, trust, code, check in pm.corruptions(good):
        dst = gm.Files()
        if code == 0:
            got = pm.unpack(dst, "f", blob, trust=trust, length=length)
            assert got["chunks_new"] == 4
            back = dst.read_complete(dst.open("f"))
            diff = np.nonzero(back != data)[0].tolist()
            assert diff == [100, 249]  # the flipped byte of chunk 1, read back through both of its spans
            continue
        with pytest.raises(pm.PackError) as e:
            pm.unpack(dst, "f", blob, trust=trust, length=length)
        assert (e.value.code, e.value.check) == (code, check), label
        assert dst.files == {} and dst.store.db == {} and dst.store.chunks_written == 0, label
        seen.add(check)
    # the list reaches every check but the two a single edit cannot reach alone
    assert set(pm.CHECKS) - seen == {"section sizes", "span_chunk of a first occurrence", "data_bytes",
                                     "external_spans"}


def test_the_checks_a_single_listed_edit_does_not_reach():
    data, chunks = pm.corrupt_source()
    src, h = written("f", data, chunks)
    good, _ = pm.pack(src, h)
    hdr, lay = pm.check_header(good, len(good))
    p = pm.Parsed(good, hdr, lay)
    edits = {
        "section sizes": pm._set_u64(good, 48, p.data_bytes + 8),
        "span_chunk of a first occurrence": pm._set_u64(good, lay["span_chunk"], pm.EXTERNAL),
        "data_bytes": pm._set_u64(pm._set_u64(good, 48, p.data_bytes + 16), 56, p.total + 16) + bytes(16),
        "external_spans": pm._set_u64(good, 40, 1),
    }
    for check, blob in edits.items():
        with pytest.raises(pm.PackError) as e:
            pm.unpack(gm.Files(), "f", blob)
        assert (e.value.code, e.value.check) == (pm.EINVAL, check)
    huge = pm.HEADER.pack(pm.MAGIC, 1, 0, 0, 1 << 60, 0, 0, 0, 64)
    with pytest.raises(pm.PackError) as e:
        pm.unpack(gm.Files(), "f", huge)
    assert e.value.check == "section sizes"
