"""CPU suite of packs (include/chunkfs_amd.h, "Packs: send and receive"): the two
symbols, the stats struct, the flag, the ctypes binding, the mirrors, the
documents, the argument checks that need no device, and the pack's arithmetic
(chunkfs_amd/csrc/pack_plan.hpp) under the address and undefined-behaviour
sanitizers as a stand-alone program.  The behaviour is in tests/test_gpu_pack.py,
the model it is compared with in tests/test_pack_model.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")
SYMBOLS = ("cdc_file_pack_device", "cdc_files_unpack_device")
FIELDS = ["spans", "chunks", "external_spans", "chunk_bytes", "pack_bytes", "file_size", "chunks_new", "seconds"]

C_SRC = r"""
#include <stddef.h>
#include "chunkfs_amd.h"
int main(void) {
    cdc_pack_stats_t st;
    int64_t (*pk)(cdc_fh_t *, cdc_fh_t *, const uint8_t *, uint8_t *, size_t, cdc_pack_stats_t *, void *) =
        cdc_file_pack_device;
    int64_t (*up)(cdc_files_t *, const char *, const uint8_t *, size_t, cdc_handle_t *, uint32_t, cdc_pack_stats_t *,
                  void *) = cdc_files_unpack_device;
    st.chunks = 7;
    if (pk(0, 0, 0, 0, 0, &st, 0) != CDC_EINVAL || pk(0, 0, 0, (uint8_t *)8, 64, &st, 0) != CDC_EINVAL) return 1;
    if (up(0, "a", 0, 64, 0, CDC_UNPACK_TRUST, &st, 0) != CDC_EINVAL) return 1;
    if (up(0, "a", 0, 64, 0, CDC_UNPACK_TRUST << 1, &st, 0) != CDC_EINVAL || st.chunks != 7) return 1;
    if (offsetof(cdc_pack_stats_t, seconds) != 56 || offsetof(cdc_pack_stats_t, chunk_bytes) != 24) return 1;
    if (offsetof(cdc_pack_stats_t, chunks_new) != 48 || offsetof(cdc_pack_stats_t, spans) != 0) return 1;
    return sizeof st == 64 && CDC_UNPACK_TRUST == 1u && CHUNKFS_AMD_ABI_VERSION == 6 ? 0 : 1;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates File::pack and Files::unpack; never run.
uint64_t use(chunkfs_amd::Files &fs, chunkfs_amd::File &a, chunkfs_amd::File &b, chunkfs_amd::Chunker &ch,
             uint8_t *d) {
    cdc_pack_stats_t st{};
    const int64_t need = a.pack(nullptr, 0), got = a.pack(d, 4096, &b, d, &st);
    const cdc_pack_stats_t x = fs.unpack("c", d, 4096, &ch), y = fs.unpack("d", d, 4096, nullptr, CDC_UNPACK_TRUST);
    return (uint64_t)need + (uint64_t)got + st.chunks + x.chunks_new + y.external_spans;
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096);
        chunkfs_amd::Files fs(st);
        chunkfs_amd::FSChunker ch(512);
        chunkfs_amd::File a = fs.create_file("a"), b = fs.create_file("b");
        return (int)use(fs, a, b, ch, nullptr);
    }
    return 0;
}
"""


def test_symbols_are_declared_listed_and_exported():
    from chunkfs_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (cdc_[a-z0-9_]+)$", out, flags=re.M))
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, txt), sym
        assert sym in _lib.EXPORTS and sym in exported, sym
    assert "cdc_pack_stats_t" in txt and re.search(r"#define\s+CDC_UNPACK_TRUST\s+1u", txt)


def test_header_states_the_contract_and_keeps_the_abi_number():
    txt = open(HEADER).read()
    assert "#define CHUNKFS_AMD_ABI_VERSION 6" in txt
    since = txt.split("Added since", 1)[1].split("*/", 1)[0]
    for sym in SYMBOLS + ("cdc_pack_stats_t", "CDC_UNPACK_TRUST"):
        assert sym in since, sym
    doc = " ".join(txt.split("/* ---- Packs: send and receive", 1)[1].split("typedef struct cdc_pack_stats", 1)[0]
                   .replace("*", " ").split())
    for words in ('the bytes "CDCPACK1"', "version = 1", "every section at a 16-byte multiple",
                  "Every padding byte, between sections and after each chunk, is zero", "byte-identical",
                  "in order of first occurrence", "Length-0 spans are legal", "its header alone, 64 bytes",
                  "some span of `since` names it", "d_have[i] != 0", "since == fh is legal and carries nothing",
                  "a return > cap means NOTHING was written", "cap = 0 sizes a pack without copying a data byte",
                  "Cursors are untouched", "The host waits for the device twice", "a misaligned d_pack",
                  "The pack is untrusted input", "no kernel reads outside [d_pack, d_pack + len)",
                  "every one before the first write to the store or the layer", "unknown flag bits", "len < 64",
                  "chunk_span strictly increasing and < n_spans", "span_chunk[chunk_span[k]] == k",
                  "chunk_off[n_chunks] == data_bytes", "the lengths sum to file_size",
                  "external_spans counts the ~0 entries", "naming the first missing span",
                  "a corrupted data byte is stored as it is", "as if every chunk were new", "First insert wins",
                  "arena_used included", "CDC_ENOTFOUND", "CDC_EEXIST", "CDC_ENOTSUP"):
        assert words in doc, words


def test_stats_struct_and_argtypes():
    from chunkfs_amd import _lib
    S = _lib.cdc_pack_stats_t
    assert ctypes.sizeof(S) == 64 and [n for n, _ in S._fields_] == FIELDS
    assert all(ctypes.sizeof(t) == 8 for _, t in S._fields_)
    assert [getattr(S, n).offset for n in FIELDS] == list(range(0, 64, 8))
    assert S._fields_[-1][1] is ctypes.c_double and all(t is ctypes.c_uint64 for _, t in S._fields_[:-1])
    assert _lib.CDC_UNPACK_TRUST == 1
    L, P, sz = _lib.lib(), ctypes.c_void_p, ctypes.c_size_t
    assert L.cdc_file_pack_device.argtypes == [P, P, P, P, sz, ctypes.POINTER(S), P]
    assert L.cdc_file_pack_device.restype is ctypes.c_int64
    assert L.cdc_files_unpack_device.argtypes == [P, ctypes.c_char_p, P, sz, P, ctypes.c_uint32, ctypes.POINTER(S), P]
    assert L.cdc_files_unpack_device.restype is ctypes.c_int64


def test_null_flag_alignment_and_length_refusals_need_no_device_and_leave_stats_alone():
    from chunkfs_amd import _lib
    L, E = _lib.lib(), _lib.CDC_EINVAL
    st = _lib.cdc_pack_stats_t(chunks=7, spans=9)
    ref = ctypes.byref(st)
    P = ctypes.c_void_p
    assert L.cdc_file_pack_device(None, None, None, None, 0, ref, None) == E
    assert b"NULL file handle" in L.cdc_last_error()
    for ptr in (1, 8, 24, (1 << 40) + 15):
        assert L.cdc_file_pack_device(None, None, None, P(ptr), 64, ref, None) == E
        assert b"not 16-byte aligned" in L.cdc_last_error()
    for flags in (2, 3, 1 << 31):
        assert L.cdc_files_unpack_device(None, b"a", None, 64, None, flags, ref, None) == E
        assert b"unknown flag bits" in L.cdc_last_error()
    for ptr in (4, 17):
        assert L.cdc_files_unpack_device(None, b"a", P(ptr), 64, None, 1, ref, None) == E
        assert b"not 16-byte aligned" in L.cdc_last_error()
    for length in (0, 1, 63):
        assert L.cdc_files_unpack_device(None, b"a", P(1 << 20), length, None, 1, ref, None) == E
        assert b"len < 64" in L.cdc_last_error()
    assert L.cdc_files_unpack_device(None, b"a", P(1 << 20), 64, None, 1, ref, None) == E
    assert b"NULL argument" in L.cdc_last_error()
    assert L.cdc_files_unpack_device(None, None, None, 64, None, 0, ref, None) == E
    assert (st.chunks, st.spans) == (7, 9)


def test_header_compiles_as_c99_and_the_struct_is_64_bytes(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_pack_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_cpp_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "pack_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "pack_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0


def test_python_mirrors_exist():
    import chunkfs_amd as c
    for fn in (c.FileSystem.pack, c.FileSystem.unpack, c.FileSystem.send, c.FileSystem.save_file,
               c.FileSystem.load_file, c.FileSystem.pack_device, c.FileSystem.unpack_device):
        assert callable(fn)
    s = c.PackStats(chunks=2, pack_bytes=96, seconds=0.5)
    assert s.chunks == 2 and s.as_dict()["pack_bytes"] == 96 and s.seconds == 0.5
    assert list(s.as_dict()) == FIELDS and "PackStats" in c.__all__


def test_the_model_names_the_checks_as_the_plan_header_does():
    import pack_model as pm
    txt = open(os.path.join(ROOT, "chunkfs_amd", "csrc", "pack_plan.hpp")).read()
    assert tuple(re.findall(r'case kPack\w+Check: return "([^"]+)";', txt)) == pm.CHECKS


def test_the_documents_name_them():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, doc)).read()
        for sym in SYMBOLS:
            assert sym in txt, (doc, sym)
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())  # whatever the line breaks
    assert "## Packs: send and receive" in design and "| f3i packs" in design
    scope = design.split("## Packs: send and receive", 1)[1]
    for words in ("several files in one pack", "packs of a scrubbed store", "compression", "streaming pack",
                  "network transport"):
        assert words in design.split("ut of scope", 1)[1] or words in scope, words
    assert "profiles/store_bench.json" in scope
    assert "examples/files_pack_example.cpp" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "examples", "files_pack_example.cpp"))
    build = open(os.path.join(ROOT, "chunkfs_amd", "build.py")).read()
    assert '"pack.hip"' in build and '"pack_plan.hpp"' in build and '"pack.hpp"' in build


def test_pack_arithmetic_under_the_host_sanitizers(tmp_path):
    """pack_plan.hpp is header-only and free of HIP: a stand-alone program with
    its own main runs it against brute force under ASan and UBSan."""
    exe = str(tmp_path / "pack_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "chunkfs_amd", "csrc"),
                    os.path.join(ROOT, "tools", "pack_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pack plan ok" in r.stdout, r.stdout + r.stderr
