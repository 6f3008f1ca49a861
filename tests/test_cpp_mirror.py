"""C++ host mirror (include/chunkfs_amd.hpp) over the C ABI.

CPU: the header-only mirror and the example compile and link against
libchunkfs_amd.so.  GPU: the example runs (FSChunker known answer, FastCDC
tiling, write-path segmentation invariance)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "_build", "cdc_example")


def _build_example():
    from chunkfs_amd import _lib  # ensures the library exists
    assert os.path.exists(_lib.LIB_PATH)
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "cdc_example.cpp"),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", EXE], check=True)


def test_cpp_mirror_compiles_and_links():
    _build_example()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_cpp_mirror_runs_on_gpu():
    _build_example()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Fixed size chunking" in r.stdout and "write path" in r.stdout


def test_cpp_mirror_throws_on_unordered_fastcdc_sizes(tmp_path):
    """The size check runs before the device is touched, so the mirror's
    constructor throws chunkfs_amd::Error(CDC_EINVAL) without a GPU too."""
    from chunkfs_amd import _lib
    src = tmp_path / "unordered.cpp"
    src.write_text('''#include <cstring>
#include "chunkfs_amd.hpp"
int main() {
    const chunkfs_amd::SizeParams bad[3] = {{1048576, 256, 1024}, {2048, 1024, 1024}, {64, 4194304, 1024}};
    for (const auto &s : bad) {
        try {
            chunkfs_amd::FastChunker c(s);
            return 1;
        } catch (const chunkfs_amd::Error &e) {
            if (e.code() != CDC_EINVAL || !std::strstr(e.what(), "max must be >= min and >= avg")) return 2;
        }
    }
    return 0;
}
''')
    exe = str(tmp_path / "unordered")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0
