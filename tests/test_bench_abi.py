"""CPU suite of the bench fixture's interface (include/chunkfs_amd.h, "Bench
fixture"): the three symbols, the C and C++ headers, the Python mirrors and the
argument checks that need no device.  No compute calls are made here."""
import ctypes
import math
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")

BENCH_SYMBOLS = ["cdc_files_get_to_dedup_ratio", "cdc_file_verify_device", "cdc_store_size_distribution_device"]

C_SRC = r"""
#include "chunkfs_amd.h"
int main(void) {
    char name[8];
    uint64_t diff = 5;
    int64_t (*ratio)(cdc_files_t *, const char *, double, char *, size_t, void *) = cdc_files_get_to_dedup_ratio;
    int64_t (*verify)(cdc_fh_t *, const uint8_t *, size_t, uint64_t *, void *) = cdc_file_verify_device;
    int64_t (*dist)(cdc_store_t *, uint64_t, uint64_t *, uint32_t *, size_t, void *) =
        cdc_store_size_distribution_device;
    if (ratio(0, "a", 2.0, name, sizeof name, 0) != CDC_EINVAL) return 1;
    if (verify(0, 0, 0, &diff, 0) != CDC_EINVAL || diff != 5) return 2;
    if (dist(0, 1, 0, 0, 0, 0) != CDC_EINVAL) return 3;
    return CHUNKFS_AMD_ABI_VERSION == 6 ? 0 : 4;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates the bench methods of the Store / Files / File mirrors; never run.
int64_t use(chunkfs_amd::Store &st, chunkfs_amd::Files &fs, const uint8_t *d, uint64_t *sizes, uint32_t *counts) {
    const std::string name = fs.get_to_dedup_ratio("a", 2.0);
    chunkfs_amd::File f = fs.open_file_readonly(name);
    uint64_t diff = 0;
    const bool same = f.verify_device(d, 0, &diff) && f.verify_device(d, 0);
    return st.size_distribution_device(4096, sizes, counts, 0) + (int64_t)diff + same + (int64_t)name.size();
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096);
        chunkfs_amd::Files fs(st);
        return (int)use(st, fs, nullptr, nullptr, nullptr);
    }
    return 0;
}
"""


def test_every_bench_symbol_is_declared_listed_and_exported():
    from chunkfs_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (cdc_[a-z0-9_]+)$", out, flags=re.M))
    for name in BENCH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS and name in exported, name
        assert hasattr(_lib.lib(), name)
        assert getattr(_lib.lib(), name).restype is ctypes.c_int64


def test_header_section_states_the_contract():
    txt = open(HEADER).read()
    sec = txt.split("---- Bench fixture", 1)[1].split("---- Synthetic data", 1)[0]
    assert "file_layer.rs:208-268" in sec and "bench/mod.rs:241-275" in sec and "bench/mod.rs:218-232" in sec
    assert "true byte position" in sec  # the one deviation: offsets in a derived file
    for refusal in ("NaN or infinite", "never end", "adjustment == 0"):  # the three refusals the reference lacks
        assert refusal in sec, refusal
    assert "NOT written" in sec and "still created" in sec  # a too-small name buffer
    assert "unwrap_chunk" in sec  # target-kind containers are counted
    assert "never reads outside" in sec
    m = re.search(r"#define CHUNKFS_AMD_ABI_VERSION (\d+)", txt)
    assert m and int(m.group(1)) == 6
    assert "cdc_store_size_distribution_device" in txt.split("#define CHUNKFS_AMD_ABI_VERSION", 1)[0]


def test_bench_header_compiles_as_c99(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_bench_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_cpp_bench_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "bench_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "bench_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0


def test_null_and_bad_arguments_are_invalid():
    from chunkfs_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the checks below come first
    buf = ctypes.create_string_buffer(16)
    assert L.cdc_files_get_to_dedup_ratio(None, b"a", 2.0, buf, 16, None) == _lib.CDC_EINVAL
    assert b"NULL" in L.cdc_last_error()
    assert L.cdc_files_get_to_dedup_ratio(fake, None, 2.0, buf, 16, None) == _lib.CDC_EINVAL
    assert L.cdc_files_get_to_dedup_ratio(fake, b"a", 2.0, None, 16, None) == _lib.CDC_EINVAL
    for ratio in (0.99, 0.0, -3.0, math.nan, math.inf, -math.inf):
        assert L.cdc_files_get_to_dedup_ratio(fake, b"a", ratio, buf, 16, None) == _lib.CDC_EINVAL, ratio
    assert b"bigger than 1" in L.cdc_last_error()  # the reference's message
    assert L.cdc_files_get_to_dedup_ratio(fake, b"a", math.inf, buf, 16, None) == _lib.CDC_EINVAL
    assert b"finite" in L.cdc_last_error()
    assert buf.raw == b"\0" * 16
    diff = ctypes.c_uint64(7)
    assert L.cdc_file_verify_device(None, None, 0, ctypes.byref(diff), None) == _lib.CDC_EINVAL
    assert b"NULL" in L.cdc_last_error() and diff.value == 7
    assert L.cdc_store_size_distribution_device(None, 1, None, None, 0, None) == _lib.CDC_EINVAL
    assert b"NULL" in L.cdc_last_error()
    assert L.cdc_store_size_distribution_device(fake, 0, None, None, 0, None) == _lib.CDC_EINVAL
    assert b"adjustment" in L.cdc_last_error()


def test_python_mirror_names():
    import chunkfs_amd as c
    from chunkfs_amd import bench
    for name in ("get_to_dedup_ratio", "verify_device", "write_from_stream"):
        assert hasattr(c.FileSystem, name)
    assert hasattr(c.ChunkStore, "size_distribution")
    for name in ("Dataset", "TimeMeasurement", "Throughput", "MeasureResult", "DedupMeasurement", "CDCFixture",
                 "VerifyError"):
        assert hasattr(bench, name)
    for name in ("fill_with", "measure", "measure_multi", "measure_repeated", "dedup_ratio", "size_distribution",
                 "chunk_count", "verify"):
        assert hasattr(bench.CDCFixture, name)


def test_dataset_reads_its_size_once(tmp_path):
    from chunkfs_amd.bench import Dataset
    path = tmp_path / "d.bin"
    path.write_bytes(b"x" * 1234)
    d = Dataset(str(path), "d")
    assert (d.size, d.name, d.path) == (1234, "d", str(path))
    with d.open() as f:
        assert f.read() == b"x" * 1234
