"""CPU suite of removal and collection (include/chunkfs_amd.h, "Removal and
collection"): the three symbols, the stats struct, the ctypes binding, the
mirrors' headers and the argument checks that need no device.  No compute calls
are made here; the behaviour is in tests/test_gpu_gc.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")
SYMBOLS = ("cdc_files_remove", "cdc_files_collect", "cdc_store_retain_device")
FIELDS = ["containers_before", "containers_after", "arena_used_before", "arena_used_after", "bytes_moved",
          "groups_direct", "groups_bounced", "seconds"]

C_SRC = r"""
#include <stddef.h>
#include "chunkfs_amd.h"
int main(void) {
    cdc_collect_stats_t st;
    int (*rm)(cdc_files_t *, const char *) = cdc_files_remove;
    int (*gc)(cdc_files_t *, cdc_collect_stats_t *, void *) = cdc_files_collect;
    int64_t (*keep)(cdc_store_t *, const uint8_t *, size_t, void *) = cdc_store_retain_device;
    st.containers_before = 7;
    if (rm(0, "x") != CDC_EINVAL || gc(0, &st, 0) != CDC_EINVAL || keep(0, 0, 0, 0) != CDC_EINVAL) return 1;
    if (st.containers_before != 7) return 1;
    if (offsetof(cdc_collect_stats_t, seconds) != 56 || offsetof(cdc_collect_stats_t, bytes_moved) != 32) return 1;
    return sizeof st == 64 && CHUNKFS_AMD_ABI_VERSION == 6 ? 0 : 1;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates Files::remove, Files::collect and Store::retain_device; never run.
uint64_t use(chunkfs_amd::Store &st, chunkfs_amd::Files &fs, const uint8_t *d) {
    fs.remove("a");
    const cdc_collect_stats_t r = fs.collect();
    return r.containers_after + r.groups_direct + r.groups_bounced + (uint64_t)st.retain_device(d, 0);
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096);
        chunkfs_amd::Files fs(st);
        return (int)use(st, fs, nullptr);
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


def test_header_states_the_contract_and_keeps_the_abi_number():
    txt = open(HEADER).read()
    assert "#define CHUNKFS_AMD_ABI_VERSION 6" in txt
    since = txt.split("Added since", 1)[1].split("*/", 1)[0]
    for sym in SYMBOLS + ("cdc_collect_stats_t",):
        assert sym in since, sym
    doc = " ".join(txt.split("/* ---- Removal and collection", 1)[1].split("typedef struct cdc_collect_stats", 1)[0]
                   .replace("*", " ").split())
    for words in ("if and only if refs > 0", "relative arena order", "sum of refs", "epoch is bumped",
                  "SECOND LAYER ON THE SAME STORE IS NOT CONSULTED", "A refused call changes nothing",
                  "CDC_ENOTSUP", "CDC_ENOTFOUND", "CDC_ENOMEM", "only for cdc_store_clear or cdc_store_destroy",
                  "CHUNKFS_AMD_GC_BOUNCE", "nothing to drop"):
        assert words in doc, words


def test_stats_struct_and_argtypes():
    from chunkfs_amd import _lib
    S = _lib.cdc_collect_stats_t
    assert ctypes.sizeof(S) == 64
    assert [n for n, _ in S._fields_] == FIELDS
    assert all(ctypes.sizeof(t) == 8 for _, t in S._fields_)
    assert S._fields_[-1][1] is ctypes.c_double and S.seconds.offset == 56
    L, P = _lib.lib(), ctypes.c_void_p
    assert L.cdc_files_remove.argtypes == [P, ctypes.c_char_p] and L.cdc_files_remove.restype is ctypes.c_int
    assert L.cdc_files_collect.argtypes == [P, ctypes.POINTER(S), P] and L.cdc_files_collect.restype is ctypes.c_int
    assert L.cdc_store_retain_device.argtypes == [P, P, ctypes.c_size_t, P]
    assert L.cdc_store_retain_device.restype is ctypes.c_int64


def test_null_arguments_are_refused_without_a_device():
    from chunkfs_amd import _lib
    L = _lib.lib()
    st = _lib.cdc_collect_stats_t(containers_before=7)
    assert L.cdc_files_remove(None, b"x") == _lib.CDC_EINVAL
    assert b"NULL argument" in L.cdc_last_error()
    assert L.cdc_files_collect(None, ctypes.byref(st), None) == _lib.CDC_EINVAL
    assert b"NULL file layer" in L.cdc_last_error()
    assert L.cdc_files_collect(None, None, None) == _lib.CDC_EINVAL
    assert L.cdc_store_retain_device(None, None, 0, None) == _lib.CDC_EINVAL
    assert b"NULL store" in L.cdc_last_error()
    assert L.cdc_store_retain_device(None, None, 3, None) == _lib.CDC_EINVAL
    assert st.containers_before == 7
    # the per-pass split of the last collect (chunkfs_amd_debug.h): six figures, none before a collect
    split = (ctypes.c_double * 6)(*[7.0] * 6)
    assert "cdc_debug_collect_split" in _lib.DEBUG_EXPORTS
    assert L.cdc_debug_collect_split(None, 0) == 6 and L.cdc_debug_collect_split(None, 2) == _lib.CDC_EINVAL
    assert L.cdc_debug_collect_split(split, 2) == 6 and list(split) == [0.0, 0.0, 7.0, 7.0, 7.0, 7.0]


def test_header_compiles_as_c99_and_the_struct_is_64_bytes(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_gc_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_cpp_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "gc_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "gc_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0


def test_python_mirrors_exist():
    import chunkfs_amd as c
    for fn in (c.FileSystem.remove_file, c.FileSystem.collect, c.ChunkStore.retain_device, c.ChunkStore.retain):
        assert callable(fn)


def test_the_knob_is_documented():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, doc)).read()
        for sym in SYMBOLS:
            assert sym in txt, (doc, sym)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Removal and collection" in design
    assert "| `CHUNKFS_AMD_GC_BOUNCE=bytes` |" in design.split("## Experiment knobs", 1)[1]
