"""CPU suite of the device chunk store's interface (include/chunkfs_amd.h,
"Chunk store"): constants, struct sizes, the C and C++ headers, and the loud
failure without a GPU.  No compute calls are made here."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates every method of the Store mirror; never run.
int64_t use(chunkfs_amd::Store &st, const uint8_t *d, const cdc_chunk_t *c, uint8_t *o, cdc_chunk_t *sp) {
    const uint8_t *streams[1] = {d};
    const uint64_t lens[1] = {0}, first[2] = {0, 0};
    int64_t r = st.put_device(d, 0, c, d, 0, o, nullptr);
    r += st.put_batch_device(1, streams, lens, first, c, d, o, nullptr);
    r += st.get_device(d, 0, o, 0, sp, nullptr);
    r += st.contains_device(d, 0, o, nullptr);
    st.clear();
    const cdc_store_stats_t s = st.stats();
    return r + (int64_t)s.arena_used + (st.handle() != nullptr);
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096);
        return (int)use(st, nullptr, nullptr, nullptr, nullptr);
    }
    return 0;
}
"""


def test_enotfound_is_minus_five():
    from chunkfs_amd import _lib
    m = re.search(r"#define CDC_ENOTFOUND \((-?\d+)\)", open(HEADER).read())
    assert m and int(m.group(1)) == -5
    assert _lib.CDC_ENOTFOUND == -5


def test_store_stats_struct_is_48_bytes():
    from chunkfs_amd import _lib
    assert ctypes.sizeof(_lib.cdc_store_stats_t) == 48


def test_store_header_compiles_as_c99(tmp_path):
    src = ('#include "chunkfs_amd.h"\n'
           "int main(void){cdc_store_stats_t s;int64_t (*g)(cdc_store_t*,const uint8_t*,size_t,uint8_t*,size_t,"
           "cdc_chunk_t*,void*)=cdc_store_get_device;(void)g;s.arena_used=0;"
           "return sizeof s==48&&s.arena_used==0&&CDC_ENOTFOUND==-5?0:1;}\n")
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_store_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=src.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_store_create_rejects_null_out():
    from chunkfs_amd import _lib
    L = _lib.lib()
    assert L.cdc_store_create(0, 16, 4096, None) == _lib.CDC_EINVAL
    assert b"out is NULL" in L.cdc_last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK),
                    reason="a GPU is visible: the no-GPU failure mode is not observable")
def test_store_without_gpu_fails_loudly():
    import chunkfs_amd
    with pytest.raises(chunkfs_amd.CdcError) as ei:
        chunkfs_amd.ChunkStore(16, 4096)
    assert ei.value.code == -3  # CDC_EDEVICE


def test_cpp_store_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "store_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "store_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0
