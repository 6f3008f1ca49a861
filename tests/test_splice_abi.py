"""CPU suite of the edit in place (include/chunkfs_amd.h, "Editing a file in
place"): the symbol, the stats struct, the ctypes binding, the mirrors, the
documents, the argument checks that need no device, and the host side's index
arithmetic (chunkfs_amd/csrc/splice_plan.hpp) under the address and
undefined-behaviour sanitizers as a stand-alone program.  The behaviour is in
tests/test_gpu_splice.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")
FIELDS = ["first_span", "spans_removed", "spans_inserted", "resync_offset", "size_before", "size_after", "bytes_new",
          "window_bytes", "rounds", "pad"]

C_SRC = r"""
#include <stddef.h>
#include "chunkfs_amd.h"
int main(void) {
    cdc_splice_stats_t st;
    int64_t (*fn)(cdc_fh_t *, cdc_handle_t *, uint64_t, uint64_t, const uint8_t *, size_t, cdc_splice_stats_t *,
                  void *) = cdc_file_splice_device;
    st.rounds = 7;
    if (fn(0, 0, 0, 0, 0, 0, &st, 0) != CDC_EINVAL || st.rounds != 7) return 1;
    if (offsetof(cdc_splice_stats_t, window_bytes) != 56 || offsetof(cdc_splice_stats_t, rounds) != 64) return 1;
    return sizeof st == 72 && CHUNKFS_AMD_ABI_VERSION == 6 ? 0 : 1;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates File::splice and its thin forms; never run.
uint64_t use(chunkfs_amd::File &f, chunkfs_amd::Chunker &ch, const uint8_t *d) {
    const cdc_splice_stats_t a = f.splice(ch, 1, 2, d, 3), b = f.pwrite(ch, 0, d, 4), c = f.insert(ch, 0, d, 5);
    const cdc_splice_stats_t e = f.delete_range(ch, 0, 6), g = f.truncate(ch, 7);
    return a.rounds + b.window_bytes + c.spans_inserted + e.spans_removed + g.size_after;
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096);
        chunkfs_amd::Files fs(st);
        chunkfs_amd::File f = fs.create_file("a");
        chunkfs_amd::FSChunker ch(512);
        return (int)use(f, ch, nullptr);
    }
    return 0;
}
"""


def test_symbol_is_declared_listed_and_exported():
    from chunkfs_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (cdc_[a-z0-9_]+)$", out, flags=re.M))
    assert re.search(r"\bcdc_file_splice_device\s*\(", txt) and "cdc_splice_stats_t" in txt
    assert "cdc_file_splice_device" in _lib.EXPORTS and "cdc_file_splice_device" in exported
    for sym in ("cdc_debug_splice_split", "cdc_debug_file_slots"):
        assert sym in _lib.DEBUG_EXPORTS and sym in exported, sym


def test_header_states_the_rule_and_keeps_the_abi_number():
    txt = open(HEADER).read()
    assert "#define CHUNKFS_AMD_ABI_VERSION 6" in txt
    since = txt.split("Added since", 1)[1].split("*/", 1)[0]
    assert "cdc_file_splice_device" in since and "cdc_splice_stats_t" in since
    doc = " ".join(txt.split("/* ---- Editing a file in place", 1)[1].split("typedef struct", 1)[0]
                   .replace("*", " ").split())
    for words in ("off[i0] + 8 <= offset", "among equal offsets the last", "the whole tail as one buffer",
                  "the smallest e_k >= offset + insert_len", "the smallest such j", "start + max + 8 <= end_w",
                  "4^r max + 8", "until cdc_files_collect", "CDC_EPERM", "CDC_ENOTFOUND", "CDC_ENOTSUP",
                  "no holes, no clipping", "returns 0 and touches nothing", "the put comes before any write"):
        assert words in doc, words


def test_stats_struct_and_argtypes():
    from chunkfs_amd import _lib
    S = _lib.cdc_splice_stats_t
    assert ctypes.sizeof(S) == 72 and [n for n, _ in S._fields_] == FIELDS
    assert S.window_bytes.offset == 56 and S.rounds.offset == 64 and S.rounds.size == 4
    L, P = _lib.lib(), ctypes.c_void_p
    assert L.cdc_file_splice_device.argtypes == [P, P, ctypes.c_uint64, ctypes.c_uint64, P, ctypes.c_size_t,
                                                 ctypes.POINTER(S), P]
    assert L.cdc_file_splice_device.restype is ctypes.c_int64


def test_null_arguments_are_refused_without_a_device():
    from chunkfs_amd import _lib
    L = _lib.lib()
    st = _lib.cdc_splice_stats_t(rounds=7)
    assert L.cdc_file_splice_device(None, None, 0, 0, None, 0, ctypes.byref(st), None) == _lib.CDC_EINVAL
    assert b"NULL file handle" in L.cdc_last_error()
    assert L.cdc_file_splice_device(None, None, 0, 0, None, 5, None, None) == _lib.CDC_EINVAL
    assert st.rounds == 7
    split = (ctypes.c_double * 5)(*[7.0] * 5)
    assert L.cdc_debug_splice_split(None, 0) == 5 and L.cdc_debug_splice_split(None, 2) == _lib.CDC_EINVAL
    assert L.cdc_debug_splice_split(split, 2) == 5 and list(split) == [0.0, 0.0, 7.0, 7.0, 7.0]
    assert L.cdc_debug_file_slots(None, None, None, 0) == _lib.CDC_EINVAL


def test_header_compiles_as_c99_and_the_struct_is_72_bytes(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_splice_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_cpp_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "splice_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "splice_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0


def test_python_mirrors_exist():
    import chunkfs_amd as c
    for fn in (c.FileSystem.splice, c.FileSystem.pwrite, c.FileSystem.insert, c.FileSystem.delete_range,
               c.FileSystem.truncate):
        assert callable(fn)
    s = c.SpliceStats(rounds=2, window_bytes=9)
    assert s.rounds == 2 and s.as_dict()["window_bytes"] == 9 and list(s.as_dict()) == FIELDS[:-1]


def test_the_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "cdc_file_splice_device" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Editing a file in place" in design and "| f3g editing a file in place" in design
    assert "examples/files_splice_example.cpp" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "examples", "files_splice_example.cpp"))


def test_index_arithmetic_under_the_host_sanitizers(tmp_path):
    """splice_plan.hpp is header-only and free of HIP: a stand-alone program with
    its own main runs it against brute force under ASan and UBSan."""
    exe = str(tmp_path / "splice_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "chunkfs_amd", "csrc"),
                    os.path.join(ROOT, "tools", "splice_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "splice plan ok" in r.stdout, r.stdout + r.stderr
