"""The AE chunker at the C ABI and in the mirrors, as far as no device is needed:
the export, the header as C, the validation that comes before any device call,
the default window."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")

C_SRC = r"""
#include <chunkfs_amd.h>
#include <chunkfs_amd_cdc_params.h>
#include <string.h>
int main(void) {
    cdc_handle_t *h = (cdc_handle_t *)0;
    if (CDC_ALGO_AE != 7 || CHUNKFS_AMD_ABI_VERSION != 6 || cdc_abi_version() != 6) return 1;
    if (CDC_AE_MODE_MAX != 0u || CDC_AE_MODE_MIN != 1u) return 2;
    if (cdc_ae_default_window(8192u) != 4767u || cdc_ae_default_window(1u) != 1u) return 3;
    if (cdc_ae_default_window(0xFFFFFFFFu) != 2499573582u) return 4;
    /* refused before any device call */
    if (cdc_create_ae(0u, 16384u, 4096u, 8192u, 16384u, 0, &h) != CDC_EINVAL || h) return 5;
    if (!strstr(cdc_last_error(), "window")) return 6;
    if (cdc_create_ae(2u, 0u, 4096u, 8192u, 16384u, 0, &h) != CDC_EINVAL || h) return 7;
    if (cdc_create(CDC_ALGO_AE, 0u, 8192u, 16384u, 0, &h) != CDC_EINVAL || h) return 8;
    return 0;
}
"""


def _nm():
    from chunkfs_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    return set(re.findall(r" T (cdc_[a-z0-9_]+)$", out, flags=re.M))


def test_cdc_create_ae_is_declared_listed_and_exported():
    from chunkfs_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+cdc_create_ae\s*\(\s*uint32_t mode,\s*uint32_t window,\s*uint32_t min,\s*uint32_t avg,"
                     r"\s*uint32_t max,\s*int device,\s*cdc_handle_t \*\*out\)", txt)
    assert re.search(r"\bCDC_ALGO_AE = 7\b", txt)
    assert "cdc_create_ae" in _lib.EXPORTS and "cdc_create_ae" in _nm()
    assert _lib.ALGO["ae"] == 7
    fn = _lib.lib().cdc_create_ae
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7


def test_abi_version_is_still_6():
    from chunkfs_amd import _lib
    assert re.search(r"#define CHUNKFS_AMD_ABI_VERSION 6\b", open(HEADER).read())
    assert _lib.lib().cdc_abi_version() == 6


def test_ae_header_compiles_as_c99(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_ae_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


@pytest.mark.parametrize("args, why", [
    ((0, 16384, 4096, 8192, 16384), "window + 1 > max"),
    ((0, 0xFFFFFFFF, 4096, 8192, 16384), "window + 1 overflows 32 bits"),
    ((2, 100, 4096, 8192, 16384), "mode = 2"),
    ((0, 100, 0, 8192, 16384), "min = 0"),
    ((0, 100, 9000, 8192, 16384), "min > avg"),
    ((1, 100, 4096, 8192, 8000), "avg > max"),
    ((0, 0, 100, 200, 100), "avg > max, default window"),
])
def test_bad_parameters_are_einval_before_any_device_call(args, why):
    from chunkfs_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cdc_create_ae(*args, 0, ctypes.byref(h)) == _lib.CDC_EINVAL, why
    assert not h.value and L.cdc_last_error()
    assert L.cdc_create_ae(0, 100, 4096, 8192, 16384, 0, None) == _lib.CDC_EINVAL  # out is NULL


def test_cdc_create_validates_ae_sizes_before_the_device():
    from chunkfs_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cdc_create(_lib.ALGO["ae"], 0, 8192, 16384, 0, ctypes.byref(h)) == _lib.CDC_EINVAL
    assert L.cdc_create(_lib.ALGO["ae"], 9000, 8192, 16384, 0, ctypes.byref(h)) == _lib.CDC_EINVAL
    # the default window never goes below 1: 1 + 1 > max = 1
    assert L.cdc_create(_lib.ALGO["ae"], 1, 1, 1, 0, ctypes.byref(h)) == _lib.CDC_EINVAL


def test_python_mirror():
    import chunkfs_amd as c
    assert "AeChunker" in c.__all__ and "AeMode" in c.__all__
    assert (c.AeMode.Max, c.AeMode.Min) == (0, 1)
    with pytest.raises(TypeError):
        c.AeChunker()
    assert c.ae_default_window(8192) == 4767
    assert c.ae_default_window(1) == 1
    with pytest.raises(c.CdcError) as ei:  # validated by the library, before any device call
        c.AeChunker(c.SizeParams(4096, 8192, 16384), window=16384)
    assert ei.value.code == c._lib.CDC_EINVAL
    with pytest.raises(c.CdcError):
        c.AeChunker(c.SizeParams(4096, 8192, 16384), mode=2)
    with pytest.raises(c.CdcError):
        c.AeChunker(c.SizeParams(4096, 8192, 16384), window=0)


def test_default_window_agrees_between_header_model_and_mirror():
    import ae_model
    import chunkfs_amd as c
    txt = open(os.path.join(INCLUDE, "chunkfs_amd_cdc_params.h")).read()
    assert "100000ull / 171828ull" in txt
    for avg in (1, 2, 64, 256, 1024, 8192, 65536, 0xFFFFFFFF):
        assert c.ae_default_window(avg) == ae_model.default_window(avg) == max(1, avg * 100000 // 171828)


def test_cpp_mirror_has_ae_chunker(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "ae_mirror.cpp"
    src.write_text(r"""
#include <chunkfs_amd.hpp>
int main() {
    using namespace chunkfs_amd;
    static_assert((uint32_t)AeMode::Max == 0 && (uint32_t)AeMode::Min == 1, "modes");
    try {
        AeChunker bad(SizeParams{4096, 8192, 16384}, 16384);  // window + 1 > max: refused before the device
        return 1;
    } catch (const std::exception &) {
    }
    uint32_t (AeChunker::*w)() const = &AeChunker::window;
    return w ? 0 : 2;
}
""")
    exe = str(tmp_path / "ae_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0
