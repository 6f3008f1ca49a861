"""CPU suite of the second hasher (include/chunkfs_amd.h, "The chunk hashers"):
the new names in the header, the library and the mirrors, the ABI number, the
ctypes binding, the refusals that need no device, and the pack header's hasher
bits (chunkfs_amd/csrc/pack_plan.hpp) under the host sanitizers as a stand-alone
program.  The behaviour is in tests/test_gpu_blake2sp.py and
tests/test_gpu_files_hash.py, the model in tests/test_blake2sp_model.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "chunkfs_amd.h")
SYMBOLS = ("cdc_hash_batch_device", "cdc_store_set_hash", "cdc_store_hash")
MACROS = ("CDC_HASH_SHA256", "CDC_HASH_BLAKE2SP")

C_SRC = r"""
#include "chunkfs_amd.h"
int main(void) {
    int (*hb)(cdc_handle_t *, int, size_t, const uint8_t *const *, const uint64_t *, const cdc_chunk_t *, uint8_t *,
              void *) = cdc_hash_batch_device;
    int (*sh)(cdc_store_t *, int) = cdc_store_set_hash;
    int (*gh)(const cdc_store_t *) = cdc_store_hash;
    if (hb(0, CDC_HASH_BLAKE2SP, 0, 0, 0, 0, 0, 0) != CDC_EINVAL) return 1;
    if (sh(0, CDC_HASH_BLAKE2SP) != CDC_EINVAL || gh(0) != CDC_HASH_SHA256) return 1;
    return CDC_HASH_SHA256 == 0 && CDC_HASH_BLAKE2SP == 1 && CHUNKFS_AMD_ABI_VERSION == 6 ? 0 : 1;
}
"""

CPP_SRC = r"""
#include "chunkfs_amd.hpp"
// Instantiates the mirror's new members; never run.
int use(chunkfs_amd::Store &st, chunkfs_amd::Chunker &ch, const uint8_t *const *streams, const uint64_t *first,
        const cdc_chunk_t *chunks, uint8_t *dig) {
    st.set_hash(CDC_HASH_BLAKE2SP);
    ch.hash_batch_device(st.hash(), 1, streams, first, chunks, dig);
    return st.hash();
}
int main(int argc, char **) {
    if (argc > 1000) {
        chunkfs_amd::Store st(16, 4096, 0, CDC_HASH_BLAKE2SP);
        chunkfs_amd::FSChunker ch(512);
        return use(st, ch, nullptr, nullptr, nullptr, nullptr);
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
    assert re.search(r"#define\s+CDC_HASH_SHA256\s+0\b", txt) and re.search(r"#define\s+CDC_HASH_BLAKE2SP\s+1\b", txt)
    # the SHA-256 entry points stay
    for sym in ("cdc_sha256_batch_device", "cdc_sha256_chunks_device"):
        assert sym in _lib.EXPORTS and sym in exported, sym


def test_header_lists_them_under_added_since_and_keeps_the_abi_number():
    from chunkfs_amd import _lib
    txt = open(HEADER).read()
    assert "#define CHUNKFS_AMD_ABI_VERSION 6" in txt
    since = txt.split("Added since", 1)[1].split("*/", 1)[0]
    for sym in SYMBOLS + MACROS:
        assert sym in since, sym
    assert _lib.lib().cdc_abi_version() == 6


def test_argtypes_and_constants():
    from chunkfs_amd import _lib
    L, P, sz = _lib.lib(), ctypes.c_void_p, ctypes.c_size_t
    assert L.cdc_hash_batch_device.argtypes == [P, ctypes.c_int, sz, P, P, P, P, P]
    assert L.cdc_hash_batch_device.restype is ctypes.c_int
    assert L.cdc_store_set_hash.argtypes == [P, ctypes.c_int] and L.cdc_store_set_hash.restype is ctypes.c_int
    assert L.cdc_store_hash.argtypes == [P] and L.cdc_store_hash.restype is ctypes.c_int
    assert (_lib.CDC_HASH_SHA256, _lib.CDC_HASH_BLAKE2SP) == (0, 1)
    assert _lib.HASH == {"sha256": 0, "blake2sp": 1}
    assert _lib.hash_code("blake2sp") == 1 and _lib.hash_code(0) == 0
    try:
        _lib.hash_code("md5")
    except ValueError as e:
        assert "md5" in str(e)
    else:
        raise AssertionError("an unknown hasher's name was accepted")


def test_refusals_that_need_no_device():
    from chunkfs_amd import _lib
    L, E = _lib.lib(), _lib.CDC_EINVAL
    for code in (0, 1):
        assert L.cdc_hash_batch_device(None, code, 0, None, None, None, None, None) == E
        assert b"NULL handle" in L.cdc_last_error()
        assert L.cdc_store_set_hash(None, code) == E
        assert b"cdc_store_set_hash: NULL store" in L.cdc_last_error()
    for code in (2, 255, 256, -1):
        assert L.cdc_hash_batch_device(None, code, 0, None, None, None, None, None) == E
        assert b"cdc_hash_batch_device: unknown hasher %d" % code in L.cdc_last_error()
        assert L.cdc_store_set_hash(None, code) == E
        assert b"cdc_store_set_hash: unknown hasher" in L.cdc_last_error()
    assert L.cdc_store_hash(None) == _lib.CDC_HASH_SHA256


def test_header_compiles_as_c99(tmp_path):
    from chunkfs_amd import _lib
    exe = str(tmp_path / "_hash_c_test")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe,
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)], input=C_SRC.encode(), check=True)
    assert subprocess.call([exe]) == 0


def test_cpp_mirror_compiles_and_links(tmp_path):
    from chunkfs_amd import _lib
    src = tmp_path / "hash_mirror.cpp"
    src.write_text(CPP_SRC)
    exe = str(tmp_path / "hash_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INCLUDE, str(src),
                    "-L", os.path.dirname(_lib.LIB_PATH), "-lchunkfs_amd",
                    "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe], check=True)
    assert subprocess.call([exe]) == 0


def test_python_mirrors_exist():
    import inspect

    import chunkfs_amd as c
    from chunkfs_amd.bench import CDCFixture
    assert callable(c.Chunker.hash_batch_device) and callable(c.ChunkStore.set_hash)
    assert isinstance(c.ChunkStore.hash, property)
    for fn in (c.ChunkStore.__init__, c.FileSystem.__init__, c.FileSystem.new_with_scrubber.__func__,
               c.Chunker.hash_batch_device):
        assert "hash" in inspect.signature(fn).parameters, fn
    assert "hash" in CDCFixture.__doc__


def test_the_kernel_is_built_and_the_order_is_shared():
    csrc = os.path.join(ROOT, "chunkfs_amd", "csrc")
    build = open(os.path.join(ROOT, "chunkfs_amd", "build.py")).read()
    assert '"blake2sp.hip"' in build and '"blake2sp.hpp"' in build
    sha_hpp = open(os.path.join(csrc, "sha256.hpp")).read()
    assert "launch_sha_order" in sha_hpp and "launch_sha256" in sha_hpp
    for f in ("sha256.hip", "blake2sp.hip"):
        assert re.search(r"\blaunch_sha_order\(b, num_cus, s\)", open(os.path.join(csrc, f)).read()), f
    b2 = open(os.path.join(csrc, "blake2sp.hip")).read()
    assert "asm" not in b2 and "launch_blake2sp" in b2


def test_the_documents_name_them():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, doc)).read()
        assert "BLAKE2sp" in txt and "cdc_hash_batch_device" in txt, doc
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    assert "## Hashers" in design
    scope = design.split("ut of scope", 1)[1]
    assert "cdc_fs_write" in scope and "cdc_chunk_and_hash" in scope and "SHA-256 only" in scope


def test_pack_header_hasher_bits_under_the_host_sanitizers(tmp_path):
    """tools/pack_plan_check.cpp, a stand-alone program under ASan and UBSan:
    the accepted non-zero hasher, the mismatch in both directions, a set high
    bit."""
    src = open(os.path.join(ROOT, "tools", "pack_plan_check.cpp")).read()
    assert "pack_flags(1) == 1" in src and "1u << bit" in src
    exe = str(tmp_path / "pack_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "chunkfs_amd", "csrc"),
                    os.path.join(ROOT, "tools", "pack_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pack plan ok" in r.stdout, r.stdout + r.stderr
