"""CPU suite of the content-aligned delta (include/chunkfs_amd.h, "Content-aligned
delta"): the symbol, the two structs, the flag, the ctypes binding, the mirrors,
the documents, the argument checks that need no device, and the delta's index
arithmetic (chunkfs_amd/csrc/delta_plan.hpp) under the address and
undefined-behaviour sanitizers as a stand-alone program.  The behaviour is in
tests/test_gpu_delta.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")
SYMBOL = "cdc_files_delta_device"
FIELDS = ["ops", "bytes_copy", "bytes_literal", "bytes_literal_tables", "spans_matched", "regions", "size_a", "size_b",
          "seconds"]

C_SRC = r"""
#include <stddef.h>
#include "chunkfs_amd.h"
int main(void) {
    cdc_delta_stats_t st;
    cdc_delta_op_t op = {0, 1, CDC_DELTA_LITERAL};
    int64_t (*dl)(cdc_fh_t *, cdc_fh_t *, uint32_t, cdc_delta_op_t *, size_t, cdc_delta_stats_t *, void *) =
        cdc_files_delta_device;
    st.regions = 7;
    if (dl(0, 0, 0, 0, 0, &st, 0) != CDC_EINVAL) return 1;
    if (dl(0, 0, CDC_DELTA_TABLES_ONLY << 1, 0, 0, &st, 0) != CDC_EINVAL || st.regions != 7) return 1;
    if (offsetof(cdc_delta_stats_t, seconds) != 64 || offsetof(cdc_delta_stats_t, regions) != 40) return 1;
    if (offsetof(cdc_delta_op_t, a_off) != 16 || op.a_off + 1 != 0) return 1;
    return sizeof st == 72 && sizeof op == 24 && CDC_DELTA_TABLES_ONLY == 1u && CHUNKFS_AMD_ABI_VERSION == 6 ? 0 : 1;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates Files::delta; never run.
uint64_t use(chunkfs_amd::Files &fs, chunkfs_amd::File &a, chunkfs_amd::File &b, cdc_delta_op_t *d) {
    const chunkfs_amd::Files::Delta x = fs.delta(a, b), y = fs.delta(a, b, CDC_DELTA_TABLES_ONLY, d, 16);
    return (uint64_t)x.ops + x.stats.bytes_literal + y.stats.bytes_literal_tables + y.stats.regions;
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


def test_the_symbol_is_declared_listed_and_exported():
    from chunkfs_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (cdc_[a-z0-9_]+)$", out, flags=re.M))
    assert re.search(r"\b%s\s*\(" % SYMBOL, txt)
    assert SYMBOL in _lib.EXPORTS and SYMBOL in exported
    assert "cdc_delta_stats_t" in txt and "cdc_delta_op_t" in txt
    assert re.search(r"#define\s+CDC_DELTA_TABLES_ONLY\s+1u", txt)
    assert re.search(r"#define\s+CDC_DELTA_LITERAL\s+\(~0ull\)", txt)


def test_header_states_the_contract_and_keeps_the_abi_number():
    txt = open(HEADER).read()
    assert "#define CHUNKFS_AMD_ABI_VERSION 6" in txt
    since = txt.split("Added since", 1)[1].split("*/", 1)[0]
    for sym in (SYMBOL, "cdc_delta_op_t", "cdc_delta_stats_t", "CDC_DELTA_LITERAL", "CDC_DELTA_TABLES_ONLY"):
        assert sym in since, sym
    doc = " ".join(txt.split("/* ---- Content-aligned delta", 1)[1].split("typedef struct cdc_delta_op", 1)[0]
                   .replace("*", " ").split())
    for words in ("tile [0, size_b) exactly", "may overlap each other and appear in any order",
                  "Spans of length 0 hold no byte and take no part", "on a tie the smaller off_a[i] wins",
                  "no arena byte is read", "0 when the region begins the file",
                  "size_a - size_b when the region ends the file", "forward takes precedence",
                  "Ops of length 0 are dropped", "adjacent COPYs on one diagonal are merged",
                  "no two LITERALs are adjacent", "written only when that number is <= cap",
                  "bytes_copy + bytes_literal == size_b", "cursors are not touched", "one COPY with a_off == 0",
                  "The host waits for the device once", "unknown flag bits", "handles of two different layers",
                  "CDC_ENOTFOUND", "CDC_ENOTSUP"):
        assert words in doc, words


def test_structs_and_argtypes():
    from chunkfs_amd import _lib
    S, O = _lib.cdc_delta_stats_t, _lib.cdc_delta_op_t
    assert ctypes.sizeof(S) == 72 and [n for n, _ in S._fields_] == FIELDS
    assert all(ctypes.sizeof(t) == 8 for _, t in S._fields_)
    assert S._fields_[-1][1] is ctypes.c_double and S.seconds.offset == 64
    assert ctypes.sizeof(O) == 24 and [n for n, _ in O._fields_] == ["b_off", "len", "a_off"]
    assert _lib.CDC_DELTA_TABLES_ONLY == 1 and _lib.CDC_DELTA_LITERAL == 2 ** 64 - 1
    L, P = _lib.lib(), ctypes.c_void_p
    assert L.cdc_files_delta_device.argtypes == [P, P, ctypes.c_uint32, P, ctypes.c_size_t, ctypes.POINTER(S), P]
    assert L.cdc_files_delta_device.restype is ctypes.c_int64


def test_null_arguments_and_unknown_flags_are_refused_without_a_device():
    from chunkfs_amd import _lib
    L = _lib.lib()
    st = _lib.cdc_delta_stats_t(regions=7)
    assert L.cdc_files_delta_device(None, None, 0, None, 0, ctypes.byref(st), None) == _lib.CDC_EINVAL
    assert b"cdc_files_delta_device: NULL file handle" in L.cdc_last_error()
    for flags in (2, 3, 1 << 31):
        assert L.cdc_files_delta_device(None, None, flags, None, 0, ctypes.byref(st), None) == _lib.CDC_EINVAL
        assert b"unknown flag bits" in L.cdc_last_error()
    assert L.cdc_files_delta_device(None, None, _lib.CDC_DELTA_TABLES_ONLY, None, 5, None, None) == _lib.CDC_EINVAL
    assert b"NULL file handle" in L.cdc_last_error()
    assert st.regions == 7
    # the diff keeps refusing the bit the delta might have been: the delta is a call of its own
    assert L.cdc_files_diff_device(None, None, 2, None, 0, None, None) == _lib.CDC_EINVAL
    assert b"unknown flag bits" in L.cdc_last_error()


def test_header_compiles_as_c99_and_the_structs_are_24_and_72_bytes(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_delta_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_cpp_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "delta_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "delta_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0


def test_python_mirrors_exist():
    import chunkfs_amd as c
    for fn in (c.FileSystem.delta, c.FileSystem.delta_device, c.FileSystem.apply_delta):
        assert callable(fn)
    s = c.DeltaStats(n_ops=2, bytes_literal=9)
    assert s.n_ops == 2 and s.as_dict()["bytes_literal"] == 9 and s.ops.shape == (0, 3) and s.literals is None
    assert list(s.as_dict())[1:] == FIELDS[1:] and c.DeltaStats.LITERAL == 2 ** 64 - 1


def test_the_documents_name_it():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert SYMBOL in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Content-aligned delta" in design and "| f3j content-aligned delta" in design
    assert "no alignment is searched for" not in design.split("## Content-aligned delta", 1)[0]
    assert "examples/files_delta_example.cpp" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "examples", "files_delta_example.cpp"))
    assert "fn cdc_files_delta_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_new_sources_are_built():
    from chunkfs_amd import build
    assert "delta.hip" in build.SOURCES and {"delta.hpp", "delta_plan.hpp"} <= set(build.HEADERS)


def test_index_arithmetic_under_the_host_sanitizers(tmp_path):
    """delta_plan.hpp is header-only and free of HIP: a stand-alone program with
    its own main walks the stages against brute force under ASan and UBSan."""
    exe = str(tmp_path / "delta_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "chunkfs_amd", "csrc"),
                    os.path.join(ROOT, "tools", "delta_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "delta plan ok" in r.stdout, r.stdout + r.stderr
