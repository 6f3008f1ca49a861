"""CPU suite of snapshots and diffs (include/chunkfs_amd.h, "Snapshots and
diffs"): the two symbols, the stats struct, the flag, the ctypes binding, the
mirrors, the documents, the argument checks that need no device, and the diff's
index arithmetic (chunkfs_amd/csrc/diff_plan.hpp) under the address and
undefined-behaviour sanitizers as a stand-alone program.  The behaviour is in
tests/test_gpu_snapshot.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")
SYMBOLS = ("cdc_files_clone", "cdc_files_diff_device")
FIELDS = ["ranges", "bytes_differing", "bytes_compared", "bytes_shared", "pieces", "size_a", "size_b", "seconds"]

C_SRC = r"""
#include <stddef.h>
#include "chunkfs_amd.h"
int main(void) {
    cdc_diff_stats_t st;
    int64_t (*cl)(cdc_files_t *, const char *, const char *, void *) = cdc_files_clone;
    int64_t (*df)(cdc_fh_t *, cdc_fh_t *, uint32_t, cdc_chunk_t *, size_t, cdc_diff_stats_t *, void *) =
        cdc_files_diff_device;
    st.pieces = 7;
    if (cl(0, "a", "b", 0) != CDC_EINVAL || df(0, 0, 0, 0, 0, &st, 0) != CDC_EINVAL) return 1;
    if (df(0, 0, CDC_DIFF_TABLES_ONLY << 1, 0, 0, &st, 0) != CDC_EINVAL || st.pieces != 7) return 1;
    if (offsetof(cdc_diff_stats_t, seconds) != 56 || offsetof(cdc_diff_stats_t, pieces) != 32) return 1;
    return sizeof st == 64 && CDC_DIFF_TABLES_ONLY == 1u && CHUNKFS_AMD_ABI_VERSION == 6 ? 0 : 1;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates Files::clone and Files::diff; never run.
uint64_t use(chunkfs_amd::Files &fs, chunkfs_amd::File &a, chunkfs_amd::File &b, cdc_chunk_t *d) {
    const int64_t n = fs.clone("a", "b");
    const chunkfs_amd::Files::Diff x = fs.diff(a, b), y = fs.diff(a, b, CDC_DIFF_TABLES_ONLY, d, 16);
    return (uint64_t)n + (uint64_t)x.ranges + x.stats.bytes_compared + y.stats.bytes_shared + y.stats.pieces;
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096);
        chunkfs_amd::Files fs(st);
        chunkfs_amd::File a = fs.create_file("a"), b = fs.create_file("c");
        return (int)use(fs, a, b, nullptr);
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
    assert "cdc_diff_stats_t" in txt and re.search(r"#define\s+CDC_DIFF_TABLES_ONLY\s+1u", txt)


def test_header_states_the_contract_and_keeps_the_abi_number():
    txt = open(HEADER).read()
    assert "#define CHUNKFS_AMD_ABI_VERSION 6" in txt
    since = txt.split("Added since", 1)[1].split("*/", 1)[0]
    for sym in SYMBOLS + ("cdc_diff_stats_t", "CDC_DIFF_TABLES_ONLY"):
        assert sym in since, sym
    doc = " ".join(txt.split("/* ---- Snapshots and diffs", 1)[1].split("typedef struct cdc_diff_stats", 1)[0]
                   .replace("*", " ").split())
    for words in ("deep copy", "smallest class that holds the spans", "No put runs, no arena byte moves",
                  "statistics are unchanged", "never shows through the other", "dst == src included",
                  "common = min(size_a, size_b)", "x >= common or A[x] != B[x]", "maximal runs",
                  "no two runs touch", "written only when that number is <= cap", "Spans of length 0 add no piece",
                  "the same slot and the same start offset", "the same slot at different offsets",
                  "bytes_shared + bytes_compared == common", "No arena byte is read", "a superset of the exact answer",
                  "bytes_compared == 0", "cursors are not touched", "The host waits for the device once",
                  "unknown flag bits", "handles of two different layers", "CDC_ENOTFOUND", "CDC_EEXIST",
                  "CDC_ENOMEM", "CDC_ENOTSUP"):
        assert words in doc, words


def test_stats_struct_and_argtypes():
    from chunkfs_amd import _lib
    S = _lib.cdc_diff_stats_t
    assert ctypes.sizeof(S) == 64 and [n for n, _ in S._fields_] == FIELDS
    assert all(ctypes.sizeof(t) == 8 for _, t in S._fields_)
    assert S._fields_[-1][1] is ctypes.c_double and S.seconds.offset == 56
    assert _lib.CDC_DIFF_TABLES_ONLY == 1
    L, P = _lib.lib(), ctypes.c_void_p
    assert L.cdc_files_clone.argtypes == [P, ctypes.c_char_p, ctypes.c_char_p, P]
    assert L.cdc_files_clone.restype is ctypes.c_int64
    assert L.cdc_files_diff_device.argtypes == [P, P, ctypes.c_uint32, P, ctypes.c_size_t, ctypes.POINTER(S), P]
    assert L.cdc_files_diff_device.restype is ctypes.c_int64


def test_null_arguments_and_unknown_flags_are_refused_without_a_device():
    from chunkfs_amd import _lib
    L = _lib.lib()
    assert L.cdc_files_clone(None, b"a", b"b", None) == _lib.CDC_EINVAL
    assert b"cdc_files_clone: NULL argument" in L.cdc_last_error()
    st = _lib.cdc_diff_stats_t(pieces=7)
    assert L.cdc_files_diff_device(None, None, 0, None, 0, ctypes.byref(st), None) == _lib.CDC_EINVAL
    assert b"NULL file handle" in L.cdc_last_error()
    for flags in (2, 3, 1 << 31):
        assert L.cdc_files_diff_device(None, None, flags, None, 0, ctypes.byref(st), None) == _lib.CDC_EINVAL
        assert b"unknown flag bits" in L.cdc_last_error()
    assert L.cdc_files_diff_device(None, None, _lib.CDC_DIFF_TABLES_ONLY, None, 5, None, None) == _lib.CDC_EINVAL
    assert b"NULL file handle" in L.cdc_last_error()
    assert st.pieces == 7


def test_header_compiles_as_c99_and_the_struct_is_64_bytes(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_snapshot_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_cpp_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "snapshot_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "snapshot_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0


def test_python_mirrors_exist():
    import chunkfs_amd as c
    for fn in (c.FileSystem.clone_file, c.FileSystem.diff, c.FileSystem.diff_device):
        assert callable(fn)
    s = c.DiffStats(n_ranges=2, bytes_compared=9)
    assert s.n_ranges == 2 and s.as_dict()["bytes_compared"] == 9 and s.ranges.shape == (0, 2)
    assert list(s.as_dict())[1:] == FIELDS[1:]


def test_the_documents_name_them():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, doc)).read()
        for sym in SYMBOLS:
            assert sym in txt, (doc, sym)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Snapshots and diffs" in design and "| f3h snapshots and diffs" in design
    scope = design.split("## Snapshots and diffs", 1)[1]
    for words in ("diff on a scrubbed store", "block-granular output", "content-aligned", "rename"):
        assert words in design.split("ut of scope", 1)[1] or words in scope, words
    assert "examples/files_snapshot_example.cpp" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "examples", "files_snapshot_example.cpp"))


def test_index_arithmetic_under_the_host_sanitizers(tmp_path):
    """diff_plan.hpp is header-only and free of HIP: a stand-alone program with
    its own main runs it against brute force under ASan and UBSan."""
    exe = str(tmp_path / "diff_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "chunkfs_amd", "csrc"),
                    os.path.join(ROOT, "tools", "diff_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "diff plan ok" in r.stdout, r.stdout + r.stderr
