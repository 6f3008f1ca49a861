"""CPU suite of the file layer's batch write (include/chunkfs_amd.h,
cdc_files_write_batch_device): the symbol, the request struct, the ctypes
binding, the mirrors' headers, argument checks that need no device, and the
packing of host buffers into one upload.  No compute calls are made here.

Not shown here: CdcError(CDC_EPERM) before any upload for a read-only handle.
A handle needs a layer, a layer a store and a store a device, so that check is
in tests/test_gpu_files_batch.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")

C_SRC = r"""
#include "chunkfs_amd.h"
#include "chunkfs_amd_debug.h"
int main(void) {
    cdc_fwrite_t rq;
    uint64_t spans[1] = {7};
    int64_t (*wb)(cdc_files_t *, cdc_handle_t *, size_t, const cdc_fwrite_t *, uint64_t *, void *) =
        cdc_files_write_batch_device;
    int64_t (*blocks)(const cdc_files_t *) = cdc_debug_files_table_blocks;
    rq.fh = 0; rq.d_data = 0; rq.len = 0;
    if (wb(0, 0, 1, &rq, spans, 0) != CDC_EINVAL || spans[0] != 7) return 1;
    if (blocks(0) != CDC_EINVAL) return 1;
    return sizeof rq == 24 && CHUNKFS_AMD_ABI_VERSION == 6 ? 0 : 1;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates Files::write_batch_device; never run.
int64_t use(chunkfs_amd::Files &fs, chunkfs_amd::Chunker &ch, const uint8_t *d) {
    chunkfs_amd::File a = fs.create_file("a");
    cdc_fwrite_t rq{a.handle(), d, 0};
    uint64_t spans = 0;
    return fs.write_batch_device(ch, 1, &rq, &spans) + fs.write_batch_device(ch, 0, nullptr) + (int64_t)spans;
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096);
        chunkfs_amd::Files fs(st);
        chunkfs_amd::FSChunker ch(4096);
        return (int)use(fs, ch, nullptr);
    }
    return 0;
}
"""


def test_symbol_is_declared_listed_and_exported():
    from chunkfs_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (cdc_[a-z0-9_]+)$", out, flags=re.M))
    assert re.search(r"\bcdc_files_write_batch_device\s*\(", txt)
    assert "cdc_files_write_batch_device" in _lib.EXPORTS and "cdc_files_write_batch_device" in exported
    assert "cdc_debug_files_table_blocks" in _lib.DEBUG_EXPORTS and "cdc_debug_files_table_blocks" in exported


def test_header_states_the_contract_and_keeps_the_abi_number():
    txt = open(HEADER).read()
    assert "#define CHUNKFS_AMD_ABI_VERSION 6" in txt
    since = txt.split("Added since", 1)[1].split("*/", 1)[0]
    assert "cdc_files_write_batch_device" in since and "cdc_fwrite_t" in since
    doc = txt.split("/* n FileSystem::write_to_file calls", 1)[1].split("cdc_files_write_batch_device(", 1)[0]
    for words in ("in request order", "arena_used", "All or nothing", "CDC_EPERM", "CDC_ENOTFOUND", "len == 0"):
        assert words in doc, words


def test_request_struct_and_argtypes():
    from chunkfs_amd import _lib
    assert ctypes.sizeof(_lib.cdc_fwrite_t) == 24
    assert [(n, ctypes.sizeof(t)) for n, t in _lib.cdc_fwrite_t._fields_] == [("fh", 8), ("d_data", 8), ("len", 8)]
    assert _lib.cdc_fwrite_t.len.offset == 16
    fn = _lib.lib().cdc_files_write_batch_device
    P = ctypes.c_void_p
    assert fn.argtypes == [P, P, ctypes.c_size_t, ctypes.POINTER(_lib.cdc_fwrite_t),
                           ctypes.POINTER(ctypes.c_uint64), P]
    assert fn.restype is ctypes.c_int64
    blocks = _lib.lib().cdc_debug_files_table_blocks
    assert blocks.argtypes == [P] and blocks.restype is ctypes.c_int64


def test_null_arguments_are_refused_without_a_device():
    from chunkfs_amd import _lib
    L = _lib.lib()
    reqs = (_lib.cdc_fwrite_t * 1)()
    spans = (ctypes.c_uint64 * 1)(7)
    assert L.cdc_files_write_batch_device(None, None, 1, reqs, spans, None) == _lib.CDC_EINVAL
    assert b"NULL file layer" in L.cdc_last_error()
    assert L.cdc_files_write_batch_device(None, None, 0, None, None, None) == _lib.CDC_EINVAL
    assert spans[0] == 7
    assert L.cdc_debug_files_table_blocks(None) == _lib.CDC_EINVAL


def test_header_compiles_as_c99_and_the_struct_is_24_bytes(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_files_batch_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_cpp_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "files_batch_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "files_batch_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0


def test_packing_is_aligned_in_order_and_without_overlap():
    import chunkfs_amd as c
    lengths = [0, 1, 15, 16, 17]
    offsets, total = c.pack_offsets(lengths)
    assert offsets == [0, 0, 16, 32, 48] and total == 65
    assert all(o % 16 == 0 for o in offsets)
    taken = [(o, o + n) for o, n in zip(offsets, lengths) if n]
    assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:]))  # in order, no overlap
    assert taken[-1][1] == total
    assert c.pack_offsets([]) == ([], 0) and c.pack_offsets([0, 0]) == ([0, 0], 0)
    offsets, total = c.pack_offsets([17, 0, 1, 32, 5])
    assert offsets == [0, 32, 32, 48, 80] and total == 85


def test_python_mirrors_exist():
    import chunkfs_amd as c
    from chunkfs_amd import bench
    assert callable(c.FileSystem.write_to_files) and callable(bench.CDCFixture.fill_with_many)
