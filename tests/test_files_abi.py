"""CPU suite of the device file layer's interface (include/chunkfs_amd.h, "File
layer"): constants, struct sizes, the C and C++ headers, argument checks that
need no device, and the loud failure without a GPU.  No compute calls are made
here."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")

FILE_SYMBOLS = [
    "cdc_files_create", "cdc_files_destroy", "cdc_files_clear", "cdc_files_exists", "cdc_files_list",
    "cdc_files_create_file", "cdc_files_open", "cdc_file_close", "cdc_file_stat", "cdc_file_write_device",
    "cdc_file_append_device", "cdc_file_read_complete_device", "cdc_file_read_device", "cdc_file_pread_device",
    "cdc_files_pread_batch_device", "cdc_file_hashes_device", "cdc_file_distribution_device",
]

C_SRC = r"""
#include "chunkfs_amd.h"
int main(void) {
    cdc_files_t *fs = 0;
    cdc_fh_t *fh = 0;
    cdc_file_stat_t st;
    cdc_pread_t rq;
    int (*create)(cdc_store_t *, size_t, cdc_files_t **) = cdc_files_create;
    int64_t (*pread)(cdc_fh_t *, uint64_t, size_t, uint8_t *, void *) = cdc_file_pread_device;
    (void)pread;
    st.size = 0; st.spans = 0; st.cursor = 0; st.chunk_seconds = 0; st.hash_seconds = 0;
    rq.fh = fh; rq.offset = 0; rq.len = 0; rq.d_dst = 0;
    if (create(0, 0, &fs) != CDC_EINVAL || fs != 0) return 1;
    return sizeof st == 40 && sizeof rq == 32 && rq.fh == 0 && CDC_EEXIST == -6 && CDC_EPERM == -7 &&
           CHUNKFS_AMD_ABI_VERSION == 6 ? 0 : 1;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates every method of the Files / File mirrors; never run.
int64_t use(chunkfs_amd::Files &fs, chunkfs_amd::Chunker &ch, const uint8_t *d, const cdc_chunk_t *c, uint8_t *o,
            cdc_chunk_t *sp, uint32_t *cnt, uint64_t *len) {
    chunkfs_amd::File a = fs.create_file("a"), b = fs.create("b", false);
    chunkfs_amd::File r = fs.open_file_readonly("a"), w = fs.open_file("a");
    int64_t x = a.write_device(ch, d, 0) + b.append_device(d, 0, c, d, 0);
    x += r.read_complete_device(o, 0, sp) + r.read_device(o, 0) + r.pread_device(0, 0, o);
    x += r.hashes_device(o, 0) + r.distribution_device(o, cnt, len, 0);
    cdc_pread_t rq{r.handle(), 0, 0, o};
    uint64_t got = 0;
    fs.pread_batch_device(1, &rq, &got);
    const cdc_file_stat_t st = w.stat();
    w.close();
    chunkfs_amd::File moved = std::move(a);
    x += fs.exists("a") + (int64_t)fs.list().size() + (int64_t)st.size + (fs.handle() != nullptr);
    fs.clear();
    return x + (int64_t)got + (moved.handle() != nullptr);
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096);
        chunkfs_amd::Files fs(st);
        chunkfs_amd::FSChunker ch(4096);
        return (int)use(fs, ch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    return 0;
}
"""


def test_error_codes_match_the_header():
    from chunkfs_amd import _lib
    txt = open(HEADER).read()
    for name, value in (("CDC_EEXIST", -6), ("CDC_EPERM", -7)):
        m = re.search(r"#define %s \((-?\d+)\)" % name, txt)
        assert m and int(m.group(1)) == value
        assert getattr(_lib, name) == value


def test_struct_sizes():
    from chunkfs_amd import _lib
    assert ctypes.sizeof(_lib.cdc_file_stat_t) == 40
    assert ctypes.sizeof(_lib.cdc_pread_t) == 32


def test_every_file_symbol_is_declared_listed_and_exported():
    from chunkfs_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (cdc_[a-z0-9_]+)$", out, flags=re.M))
    for name in FILE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS and name in exported, name
        assert hasattr(_lib.lib(), name)


def test_header_section_cites_the_reference():
    txt = open(HEADER).read()
    sec = txt.split("---- File layer", 1)[1].split("---- Synthetic data", 1)[0]
    assert sec.count("file_layer.rs:") >= 10 and "mod.rs:" in sec
    assert "true byte" in sec  # the stated deviation


def test_files_header_compiles_as_c99(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_files_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_create_rejects_null_arguments():
    from chunkfs_amd import _lib
    L = _lib.lib()
    out = ctypes.c_void_p(1234)
    assert L.cdc_files_create(None, 0, ctypes.byref(out)) == _lib.CDC_EINVAL
    assert out.value is None
    assert b"store is NULL" in L.cdc_last_error()
    assert L.cdc_files_create(None, 0, None) == _lib.CDC_EINVAL
    assert b"out is NULL" in L.cdc_last_error()
    assert L.cdc_files_open(None, b"x", 0, ctypes.byref(out)) == _lib.CDC_EINVAL
    assert L.cdc_file_stat(None, None) == _lib.CDC_EINVAL
    assert L.cdc_file_read_device(None, None, 0, None) == _lib.CDC_EINVAL
    L.cdc_file_close(None)
    L.cdc_files_destroy(None)


def test_scrub_is_invalid_input_and_needs_no_device():
    import chunkfs_amd as c
    fs = c.FileSystem.__new__(c.FileSystem)  # scrub touches no state
    with pytest.raises(c.CdcError) as ei:
        fs.scrub()
    assert ei.value.code == c._lib.CDC_EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK),
                    reason="a GPU is visible: the no-GPU failure mode is not observable")
def test_filesystem_without_gpu_fails_loudly():
    import chunkfs_amd
    with pytest.raises(chunkfs_amd.CdcError) as ei:
        chunkfs_amd.FileSystem()
    assert ei.value.code == -3  # CDC_EDEVICE


def test_cpp_files_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "files_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "files_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0


def test_read_planner_arithmetic_under_the_host_sanitizers(tmp_path):
    """read_plan.hpp is header-only and free of HIP: a stand-alone program with
    its own main checks the host's bounds against what the planner resolves,
    under ASan and UBSan."""
    exe = str(tmp_path / "read_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "chunkfs_amd", "csrc"),
                    os.path.join(ROOT, "tools", "read_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "read plan ok" in r.stdout, r.stdout + r.stderr
