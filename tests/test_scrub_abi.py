"""CPU suite of the scrub stage's interface (include/chunkfs_amd.h, "Scrub
stage"): symbols, struct sizes, the C and C++ headers, and argument checks that
need no device.  No compute calls are made here."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")

SCRUB_SYMBOLS = ["cdc_store_set_target", "cdc_store_scrub", "cdc_store_scrub_stats", "cdc_store_iterate_device",
                 "cdc_store_keys_device"]

C_SRC = r"""
#include "chunkfs_amd.h"
int main(void) {
    cdc_scrub_measurements_t m;
    cdc_scrub_stats_t s;
    cdc_store_stats_t st;
    cdc_file_stat_t fst;
    cdc_pread_t rq;
    int (*scrub)(cdc_store_t *, int, cdc_handle_t *, cdc_scrub_measurements_t *, void *) = cdc_store_scrub;
    int64_t (*keys)(cdc_store_t *, uint8_t *, size_t, void *) = cdc_store_keys_device;
    (void)keys; (void)st; (void)fst; (void)rq;
    m.processed_data = 0; m.running_seconds = 0; m.data_left = 0;
    s.cdc_bytes = s.chunk_containers = s.target_containers = s.keys = s.target_bytes = s.target_values = 0;
    if (scrub(0, CDC_SCRUB_COPY, 0, &m, 0) != CDC_EINVAL) return 1;
    if (cdc_store_set_target(0, 0) != CDC_EINVAL) return 1;
    return sizeof m == 24 && sizeof s == 48 && sizeof st == 48 && sizeof fst == 40 && sizeof rq == 32 &&
           CDC_SCRUB_DUMB == 0 && CDC_SCRUB_COPY == 1 && CDC_SCRUB_RECHUNK == 2 && s.keys == 0 ? 0 : 1;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates the scrub methods of the Store / Files mirrors; never run.
int64_t use(chunkfs_amd::Store &st, chunkfs_amd::Store &tg, chunkfs_amd::Files &fs, chunkfs_amd::Chunker &ch,
            uint8_t *o, uint64_t *u) {
    st.set_target(tg);
    const cdc_scrub_measurements_t a = st.scrub(CDC_SCRUB_COPY), b = st.scrub(CDC_SCRUB_RECHUNK, &ch);
    const cdc_scrub_stats_t s = st.scrub_stats();
    int64_t x = st.iterate_device(o, o, u, u, 0) + st.keys_device(o, 0);
    fs.clear_file_system(tg);
    return x + (int64_t)(a.processed_data + b.data_left + s.keys);
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096), tg(16, 4096);
        chunkfs_amd::Files fs(st);
        chunkfs_amd::FSChunker ch(512);
        return (int)use(st, tg, fs, ch, nullptr, nullptr);
    }
    return 0;
}
"""


def test_struct_sizes_new_and_old():
    from chunkfs_amd import _lib
    assert ctypes.sizeof(_lib.cdc_scrub_measurements_t) == 24
    assert ctypes.sizeof(_lib.cdc_scrub_stats_t) == 48
    assert ctypes.sizeof(_lib.cdc_store_stats_t) == 48
    assert ctypes.sizeof(_lib.cdc_file_stat_t) == 40
    assert ctypes.sizeof(_lib.cdc_pread_t) == 32


def test_scrubber_codes_match_the_header():
    from chunkfs_amd import _lib
    txt = open(HEADER).read()
    for name, value in (("CDC_SCRUB_DUMB", 0), ("CDC_SCRUB_COPY", 1), ("CDC_SCRUB_RECHUNK", 2)):
        m = re.search(r"#define %s (\d+)" % name, txt)
        assert m and int(m.group(1)) == value == getattr(_lib, name)


def test_every_scrub_symbol_is_declared_listed_and_exported():
    from chunkfs_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (cdc_[a-z0-9_]+)$", out, flags=re.M))
    for name in SCRUB_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS and name in exported, name
        assert hasattr(_lib.lib(), name)


def test_header_section_cites_the_reference():
    txt = open(HEADER).read()
    sec = txt.split("---- Scrub stage", 1)[1].split("---- File layer", 1)[0]
    assert "scrub.rs:85-114" in sec and "scrub.rs:116-129" in sec and "scrub.rs:71-79" in sec
    assert "storage.rs:12-21" in sec and "storage.rs:141-157" in sec and "mod.rs:226-298" in sec
    assert "this project's own" in sec  # RechunkScrubber has no counterpart
    assert "64-bit key" in sec  # the index's result-dependent errors stay what they are


def test_scrub_header_compiles_as_c99(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_scrub_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_null_and_self_target_arguments_are_invalid():
    from chunkfs_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)  # compared, never dereferenced: the NULL / self checks come first
    assert L.cdc_store_set_target(None, None) == _lib.CDC_EINVAL
    assert b"NULL" in L.cdc_last_error()
    assert L.cdc_store_set_target(fake, None) == _lib.CDC_EINVAL
    assert L.cdc_store_set_target(None, fake) == _lib.CDC_EINVAL
    assert b"NULL" in L.cdc_last_error()
    assert L.cdc_store_set_target(fake, fake) == _lib.CDC_EINVAL
    assert b"own target" in L.cdc_last_error()
    m = _lib.cdc_scrub_measurements_t()
    assert L.cdc_store_scrub(None, _lib.CDC_SCRUB_COPY, None, ctypes.byref(m), None) == _lib.CDC_EINVAL
    assert b"NULL" in L.cdc_last_error()
    assert L.cdc_store_scrub_stats(None, None) == _lib.CDC_EINVAL
    assert L.cdc_store_iterate_device(None, None, None, None, None, 0, None) == _lib.CDC_EINVAL
    assert L.cdc_store_keys_device(None, None, 0, None) == _lib.CDC_EINVAL
    assert b"NULL" in L.cdc_last_error()


def test_scrub_of_a_plain_file_system_is_still_invalid_input():
    import chunkfs_amd as c
    fs = c.FileSystem.__new__(c.FileSystem)  # touches no attributes
    with pytest.raises(c.CdcError) as ei:
        fs.scrub()
    assert ei.value.code == c._lib.CDC_EINVAL


def test_python_mirror_names():
    import chunkfs_amd as c
    for name in ("CopyScrubber", "DumbScrubber", "RechunkScrubber", "ScrubMeasurements"):
        assert name in c.__all__ and hasattr(c, name)
    for name in ("new_with_scrubber", "scrub", "total_dedup_ratio", "storage_iterator", "clear_file_system"):
        assert hasattr(c.FileSystem, name)
    for name in ("set_target", "scrub", "scrub_stats", "storage_iterator"):
        assert hasattr(c.ChunkStore, name)
    m = c.ScrubMeasurements()
    assert (m.processed_data, m.running_time, m.data_left) == (0, 0.0, 0)


def test_cpp_scrub_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "scrub_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "scrub_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0
