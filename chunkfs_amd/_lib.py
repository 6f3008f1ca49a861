"""ctypes binding of libchunkfs_amd.so (include/chunkfs_amd.h).

Loading fails loudly: there is no CPU fallback anywhere in the product.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# CHUNKFS_AMD_LIB: an experiment build of the same sources (tools/scan_variants.sh)
LIB_PATH = os.environ.get("CHUNKFS_AMD_LIB") or os.path.join(HERE, "libchunkfs_amd.so")

CDC_OK = 0
CDC_EINVAL = -1
CDC_ENOMEM = -2
CDC_EDEVICE = -3
CDC_ENOTSUP = -4
CDC_ENOTFOUND = -5
CDC_EEXIST = -6
CDC_EPERM = -7

ALGO = {"fast": 0, "fixed": 1, "rabin": 2, "super": 3, "ultra": 4, "leap": 5, "seq": 6, "ae": 7}

# Every symbol include/chunkfs_amd.h declares (tests check the export table).
EXPORTS = [
    "cdc_create", "cdc_create_seq", "cdc_create_ae", "cdc_destroy", "cdc_chunk_data", "cdc_estimate_chunk_count",
    "cdc_max_chunk_count", "cdc_describe", "cdc_last_error", "cdc_set_gear", "cdc_set_rabin_poly",
    "cdc_chunk_batch_device", "cdc_chunk_batch_device_async", "cdc_batch_sync", "cdc_batch_max_chunks",
    "cdc_last_timing",
    "cdc_fs_write", "cdc_write_begin", "cdc_write_segment", "cdc_write_drain", "cdc_write_finish",
    "cdc_sha256_chunks_device", "cdc_sha256_batch_device", "cdc_chunk_and_hash",
    "cdc_index_create", "cdc_index_destroy", "cdc_index_clear", "cdc_index_insert_device",
    "cdc_index_stats",
    "cdc_store_create", "cdc_store_destroy", "cdc_store_clear", "cdc_store_stats", "cdc_store_put_device",
    "cdc_store_put_batch_device", "cdc_store_get_device", "cdc_store_contains_device",
    "cdc_store_set_target", "cdc_store_scrub", "cdc_store_scrub_stats", "cdc_store_iterate_device",
    "cdc_store_keys_device",
    "cdc_files_create", "cdc_files_destroy", "cdc_files_clear", "cdc_files_exists", "cdc_files_list",
    "cdc_files_create_file", "cdc_files_open", "cdc_file_close", "cdc_file_stat", "cdc_file_write_device",
    "cdc_file_append_device", "cdc_file_read_complete_device", "cdc_file_read_device", "cdc_file_pread_device",
    "cdc_files_pread_batch_device", "cdc_file_hashes_device", "cdc_file_distribution_device",
    "cdc_files_write_batch_device",
    "cdc_files_get_to_dedup_ratio", "cdc_file_verify_device", "cdc_store_size_distribution_device",
    "cdc_files_remove", "cdc_files_collect", "cdc_store_retain_device",
    "cdc_file_splice_device",
    "cdc_files_clone", "cdc_files_diff_device", "cdc_files_delta_device",
    "cdc_file_pack_device", "cdc_files_unpack_device",
    "cdc_hash_batch_device", "cdc_store_set_hash", "cdc_store_hash",
    "cdc_fill_splitmix64_device", "cdc_version", "cdc_abi_version",
]
# include/chunkfs_amd_debug.h (diagnostics, not part of the drop-in boundary)
DEBUG_EXPORTS = ["cdc_debug_pipeline", "cdc_debug_record_cap", "cdc_debug_copy", "cdc_debug_host_stats",
                 "cdc_debug_read_bw", "cdc_debug_host_placement",
                 "cdc_debug_timing_back", "cdc_debug_walk_params", "cdc_debug_files_table_blocks",
                 "cdc_debug_collect_split", "cdc_debug_splice_split", "cdc_debug_file_slots",
                 "cdc_debug_pack_split"]


class CdcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"chunkfs_amd error {code}: {msg}")
        self.code = code


class cdc_chunk_t(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint64)]


class cdc_index_stats_t(ctypes.Structure):
    _fields_ = [("chunks_written", ctypes.c_uint64), ("bytes_written", ctypes.c_uint64),
                ("unique_chunks", ctypes.c_uint64), ("unique_bytes", ctypes.c_uint64)]


class cdc_store_stats_t(ctypes.Structure):
    _fields_ = [("index", cdc_index_stats_t), ("arena_capacity", ctypes.c_uint64),
                ("arena_used", ctypes.c_uint64)]


class cdc_scrub_measurements_t(ctypes.Structure):
    _fields_ = [("processed_data", ctypes.c_uint64), ("running_seconds", ctypes.c_double),
                ("data_left", ctypes.c_uint64)]


class cdc_scrub_stats_t(ctypes.Structure):
    _fields_ = [("cdc_bytes", ctypes.c_uint64), ("chunk_containers", ctypes.c_uint64),
                ("target_containers", ctypes.c_uint64), ("keys", ctypes.c_uint64),
                ("target_bytes", ctypes.c_uint64), ("target_values", ctypes.c_uint64)]


CDC_SCRUB_DUMB, CDC_SCRUB_COPY, CDC_SCRUB_RECHUNK = 0, 1, 2


class cdc_file_stat_t(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint64), ("spans", ctypes.c_uint64), ("cursor", ctypes.c_uint64),
                ("chunk_seconds", ctypes.c_double), ("hash_seconds", ctypes.c_double)]


class cdc_pread_t(ctypes.Structure):
    _fields_ = [("fh", ctypes.c_void_p), ("offset", ctypes.c_uint64), ("len", ctypes.c_uint64),
                ("d_dst", ctypes.c_void_p)]


class cdc_fwrite_t(ctypes.Structure):
    _fields_ = [("fh", ctypes.c_void_p), ("d_data", ctypes.c_void_p), ("len", ctypes.c_uint64)]


class cdc_collect_stats_t(ctypes.Structure):
    _fields_ = [("containers_before", ctypes.c_uint64), ("containers_after", ctypes.c_uint64),
                ("arena_used_before", ctypes.c_uint64), ("arena_used_after", ctypes.c_uint64),
                ("bytes_moved", ctypes.c_uint64), ("groups_direct", ctypes.c_uint64),
                ("groups_bounced", ctypes.c_uint64), ("seconds", ctypes.c_double)]


class cdc_splice_stats_t(ctypes.Structure):
    _fields_ = [("first_span", ctypes.c_uint64), ("spans_removed", ctypes.c_uint64),
                ("spans_inserted", ctypes.c_uint64), ("resync_offset", ctypes.c_uint64),
                ("size_before", ctypes.c_uint64), ("size_after", ctypes.c_uint64),
                ("bytes_new", ctypes.c_uint64), ("window_bytes", ctypes.c_uint64),
                ("rounds", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class cdc_pack_stats_t(ctypes.Structure):
    _fields_ = [("spans", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("external_spans", ctypes.c_uint64),
                ("chunk_bytes", ctypes.c_uint64), ("pack_bytes", ctypes.c_uint64), ("file_size", ctypes.c_uint64),
                ("chunks_new", ctypes.c_uint64), ("seconds", ctypes.c_double)]


class cdc_diff_stats_t(ctypes.Structure):
    _fields_ = [("ranges", ctypes.c_uint64), ("bytes_differing", ctypes.c_uint64),
                ("bytes_compared", ctypes.c_uint64), ("bytes_shared", ctypes.c_uint64),
                ("pieces", ctypes.c_uint64), ("size_a", ctypes.c_uint64), ("size_b", ctypes.c_uint64),
                ("seconds", ctypes.c_double)]


CDC_DIFF_TABLES_ONLY = 1


class cdc_delta_op_t(ctypes.Structure):
    _fields_ = [("b_off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("a_off", ctypes.c_uint64)]


class cdc_delta_stats_t(ctypes.Structure):
    _fields_ = [("ops", ctypes.c_uint64), ("bytes_copy", ctypes.c_uint64), ("bytes_literal", ctypes.c_uint64),
                ("bytes_literal_tables", ctypes.c_uint64), ("spans_matched", ctypes.c_uint64),
                ("regions", ctypes.c_uint64), ("size_a", ctypes.c_uint64), ("size_b", ctypes.c_uint64),
                ("seconds", ctypes.c_double)]


CDC_DELTA_LITERAL = 0xFFFFFFFFFFFFFFFF
CDC_DELTA_TABLES_ONLY = 1
CDC_UNPACK_TRUST = 1
CDC_HASH_SHA256 = 0
CDC_HASH_BLAKE2SP = 1
HASH = {"sha256": CDC_HASH_SHA256, "blake2sp": CDC_HASH_BLAKE2SP}


def hash_code(name):
    """CDC_HASH_* of a hasher's name ("sha256" | "blake2sp") or of a code."""
    if isinstance(name, str):
        if name not in HASH:
            raise ValueError(f"unknown hasher {name!r}: one of {sorted(HASH)}")
        return HASH[name]
    return int(name)


class cdc_timing_t(ctypes.Structure):
    _fields_ = [
        ("scan_ms", ctypes.c_double),
        ("resolve_ms", ctypes.c_double),
        ("compact_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("fixup_iterations", ctypes.c_uint32),
        ("overflow_spans", ctypes.c_uint32),
        ("candidates", ctypes.c_uint64),
        ("bytes", ctypes.c_uint64),
        ("hash_ms", ctypes.c_double),
        ("walk_fallback_steps", ctypes.c_uint64),
        ("path", ctypes.c_uint32),   # CDC_PATH_*: 0 pipeline, 1 small kernel, 2 walk, 3 fixed, 4 empty
        ("timed", ctypes.c_uint32),  # 1: the *_ms fields are HIP-event measurements
    ]


_lib = None


def lib():
    """Load and type the shared library (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP engine is the only implementation; there is no CPU fallback)")
    # PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME
    # libamdhip64.so.7 as /opt/rocm's).  If ours were loaded first, a later
    # `import torch` would map a SECOND HIP runtime into the process and fail
    # ("No HIP GPUs are available").  Importing torch first makes our NEEDED
    # libamdhip64.so.7 resolve to the already-loaded copy: one runtime, shared
    # device pointers and streams.  Without torch the system runtime is used.
    if "torch" not in sys.modules and not os.environ.get("CHUNKFS_AMD_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    sz = ctypes.c_size_t
    L.cdc_create.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                             ctypes.c_int, ctypes.POINTER(P)]
    L.cdc_create.restype = ctypes.c_int
    u32 = ctypes.c_uint32
    L.cdc_create_seq.argtypes = [u32, u32, u32, u32, u32, u32, u32, ctypes.c_int, ctypes.POINTER(P)]
    L.cdc_create_seq.restype = ctypes.c_int
    L.cdc_create_ae.argtypes = [u32, u32, u32, u32, u32, ctypes.c_int, ctypes.POINTER(P)]
    L.cdc_create_ae.restype = ctypes.c_int
    L.cdc_destroy.argtypes = [P]
    L.cdc_destroy.restype = None
    L.cdc_chunk_data.argtypes = [P, P, sz, ctypes.POINTER(cdc_chunk_t), sz]
    L.cdc_chunk_data.restype = ctypes.c_int64
    L.cdc_estimate_chunk_count.argtypes = [P, sz]
    L.cdc_estimate_chunk_count.restype = sz
    L.cdc_max_chunk_count.argtypes = [P, sz]
    L.cdc_max_chunk_count.restype = sz
    L.cdc_describe.argtypes = [P]
    L.cdc_describe.restype = ctypes.c_char_p
    L.cdc_last_error.argtypes = []
    L.cdc_last_error.restype = ctypes.c_char_p
    L.cdc_set_gear.argtypes = [P, u64p]
    L.cdc_set_gear.restype = ctypes.c_int
    L.cdc_set_rabin_poly.argtypes = [P, ctypes.c_uint64]
    L.cdc_set_rabin_poly.restype = ctypes.c_int
    L.cdc_chunk_batch_device.argtypes = [P, sz, P, P, P, sz, P, P]
    L.cdc_chunk_batch_device.restype = ctypes.c_int64
    L.cdc_chunk_batch_device_async.argtypes = [P, sz, P, P, P, sz, P, P]
    L.cdc_chunk_batch_device_async.restype = ctypes.c_int64
    L.cdc_batch_sync.argtypes = [P]
    L.cdc_batch_sync.restype = ctypes.c_int64
    L.cdc_batch_max_chunks.argtypes = [P, sz, u64p]
    L.cdc_batch_max_chunks.restype = sz
    L.cdc_last_timing.argtypes = [P, ctypes.POINTER(cdc_timing_t), sz]
    L.cdc_last_timing.restype = ctypes.c_int
    L.cdc_fs_write.argtypes = [P, P, sz, sz, u64p, sz, ctypes.POINTER(ctypes.c_double)]
    L.cdc_fs_write.restype = ctypes.c_int64
    L.cdc_write_begin.argtypes = [P]
    L.cdc_write_begin.restype = ctypes.c_int
    L.cdc_write_segment.argtypes = [P, P, sz]
    L.cdc_write_segment.restype = ctypes.c_int
    L.cdc_write_drain.argtypes = [P, u64p, sz]
    L.cdc_write_drain.restype = ctypes.c_int64
    L.cdc_write_finish.argtypes = [P, u64p, sz, ctypes.POINTER(ctypes.c_double)]
    L.cdc_write_finish.restype = ctypes.c_int64
    L.cdc_debug_host_stats.argtypes = [P, ctypes.POINTER(ctypes.c_double), sz]
    L.cdc_debug_host_stats.restype = ctypes.c_int
    L.cdc_debug_timing_back.argtypes = [P, ctypes.c_uint32, ctypes.POINTER(cdc_timing_t), sz]
    L.cdc_debug_timing_back.restype = ctypes.c_int
    L.cdc_debug_walk_params.argtypes = [P, ctypes.POINTER(ctypes.c_uint64), sz]
    L.cdc_debug_walk_params.restype = ctypes.c_int
    L.cdc_sha256_chunks_device.argtypes = [P, P, P, sz, P, P]
    L.cdc_sha256_chunks_device.restype = ctypes.c_int
    L.cdc_sha256_batch_device.argtypes = [P, sz, P, P, P, P, P]
    L.cdc_sha256_batch_device.restype = ctypes.c_int
    L.cdc_chunk_and_hash.argtypes = [P, P, sz, ctypes.POINTER(cdc_chunk_t), u8p, sz]
    L.cdc_chunk_and_hash.restype = ctypes.c_int64
    L.cdc_index_create.argtypes = [ctypes.c_int, sz, ctypes.POINTER(P)]
    L.cdc_index_create.restype = ctypes.c_int
    L.cdc_index_destroy.argtypes = [P]
    L.cdc_index_destroy.restype = None
    L.cdc_index_clear.argtypes = [P]
    L.cdc_index_clear.restype = ctypes.c_int
    L.cdc_index_insert_device.argtypes = [P, P, P, sz, P, P]
    L.cdc_index_insert_device.restype = ctypes.c_int64
    L.cdc_index_stats.argtypes = [P, ctypes.POINTER(cdc_index_stats_t)]
    L.cdc_index_stats.restype = ctypes.c_int
    L.cdc_store_create.argtypes = [ctypes.c_int, sz, sz, ctypes.POINTER(P)]
    L.cdc_store_create.restype = ctypes.c_int
    L.cdc_store_destroy.argtypes = [P]
    L.cdc_store_destroy.restype = None
    L.cdc_store_clear.argtypes = [P]
    L.cdc_store_clear.restype = ctypes.c_int
    L.cdc_store_stats.argtypes = [P, ctypes.POINTER(cdc_store_stats_t)]
    L.cdc_store_stats.restype = ctypes.c_int
    L.cdc_store_put_device.argtypes = [P, P, sz, P, P, sz, P, P]
    L.cdc_store_put_device.restype = ctypes.c_int64
    L.cdc_store_put_batch_device.argtypes = [P, sz, P, P, P, P, P, P, P]
    L.cdc_store_put_batch_device.restype = ctypes.c_int64
    L.cdc_store_get_device.argtypes = [P, P, sz, P, sz, P, P]
    L.cdc_store_get_device.restype = ctypes.c_int64
    L.cdc_store_contains_device.argtypes = [P, P, sz, P, P]
    L.cdc_store_contains_device.restype = ctypes.c_int64
    L.cdc_hash_batch_device.argtypes = [P, ctypes.c_int, sz, P, P, P, P, P]
    L.cdc_hash_batch_device.restype = ctypes.c_int
    L.cdc_store_set_hash.argtypes = [P, ctypes.c_int]
    L.cdc_store_set_hash.restype = ctypes.c_int
    L.cdc_store_hash.argtypes = [P]
    L.cdc_store_hash.restype = ctypes.c_int
    L.cdc_store_set_target.argtypes = [P, P]
    L.cdc_store_set_target.restype = ctypes.c_int
    L.cdc_store_scrub.argtypes = [P, ctypes.c_int, P, ctypes.POINTER(cdc_scrub_measurements_t), P]
    L.cdc_store_scrub.restype = ctypes.c_int
    L.cdc_store_scrub_stats.argtypes = [P, ctypes.POINTER(cdc_scrub_stats_t)]
    L.cdc_store_scrub_stats.restype = ctypes.c_int
    L.cdc_store_iterate_device.argtypes = [P, P, P, P, P, sz, P]
    L.cdc_store_iterate_device.restype = ctypes.c_int64
    L.cdc_store_keys_device.argtypes = [P, P, sz, P]
    L.cdc_store_keys_device.restype = ctypes.c_int64
    L.cdc_files_create.argtypes = [P, sz, ctypes.POINTER(P)]
    L.cdc_files_create.restype = ctypes.c_int
    L.cdc_files_destroy.argtypes = [P]
    L.cdc_files_destroy.restype = None
    L.cdc_files_clear.argtypes = [P]
    L.cdc_files_clear.restype = ctypes.c_int
    L.cdc_files_exists.argtypes = [P, ctypes.c_char_p]
    L.cdc_files_exists.restype = ctypes.c_int
    L.cdc_files_list.argtypes = [P, ctypes.c_char_p, sz]
    L.cdc_files_list.restype = ctypes.c_int64
    L.cdc_files_create_file.argtypes = [P, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(P)]
    L.cdc_files_create_file.restype = ctypes.c_int
    L.cdc_files_open.argtypes = [P, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(P)]
    L.cdc_files_open.restype = ctypes.c_int
    L.cdc_file_close.argtypes = [P]
    L.cdc_file_close.restype = None
    L.cdc_file_stat.argtypes = [P, ctypes.POINTER(cdc_file_stat_t)]
    L.cdc_file_stat.restype = ctypes.c_int
    L.cdc_file_write_device.argtypes = [P, P, P, sz, P]
    L.cdc_file_write_device.restype = ctypes.c_int64
    L.cdc_file_append_device.argtypes = [P, P, sz, P, P, sz, P]
    L.cdc_file_append_device.restype = ctypes.c_int64
    L.cdc_file_read_complete_device.argtypes = [P, P, sz, P, P]
    L.cdc_file_read_complete_device.restype = ctypes.c_int64
    L.cdc_file_read_device.argtypes = [P, P, sz, P]
    L.cdc_file_read_device.restype = ctypes.c_int64
    L.cdc_file_pread_device.argtypes = [P, ctypes.c_uint64, sz, P, P]
    L.cdc_file_pread_device.restype = ctypes.c_int64
    L.cdc_files_pread_batch_device.argtypes = [P, sz, ctypes.POINTER(cdc_pread_t), u64p, P]
    L.cdc_files_pread_batch_device.restype = ctypes.c_int
    L.cdc_files_write_batch_device.argtypes = [P, P, sz, ctypes.POINTER(cdc_fwrite_t), u64p, P]
    L.cdc_files_write_batch_device.restype = ctypes.c_int64
    L.cdc_file_hashes_device.argtypes = [P, P, sz]
    L.cdc_file_hashes_device.restype = ctypes.c_int64
    L.cdc_file_distribution_device.argtypes = [P, P, P, P, sz, P]
    L.cdc_file_distribution_device.restype = ctypes.c_int64
    L.cdc_files_get_to_dedup_ratio.argtypes = [P, ctypes.c_char_p, ctypes.c_double, ctypes.c_char_p, sz, P]
    L.cdc_files_get_to_dedup_ratio.restype = ctypes.c_int64
    L.cdc_file_verify_device.argtypes = [P, P, sz, u64p, P]
    L.cdc_file_verify_device.restype = ctypes.c_int64
    L.cdc_store_size_distribution_device.argtypes = [P, ctypes.c_uint64, P, P, sz, P]
    L.cdc_store_size_distribution_device.restype = ctypes.c_int64
    L.cdc_files_remove.argtypes = [P, ctypes.c_char_p]
    L.cdc_files_remove.restype = ctypes.c_int
    L.cdc_files_collect.argtypes = [P, ctypes.POINTER(cdc_collect_stats_t), P]
    L.cdc_files_collect.restype = ctypes.c_int
    L.cdc_store_retain_device.argtypes = [P, P, sz, P]
    L.cdc_store_retain_device.restype = ctypes.c_int64
    L.cdc_file_splice_device.argtypes = [P, P, ctypes.c_uint64, ctypes.c_uint64, P, sz,
                                         ctypes.POINTER(cdc_splice_stats_t), P]
    L.cdc_file_splice_device.restype = ctypes.c_int64
    L.cdc_files_clone.argtypes = [P, ctypes.c_char_p, ctypes.c_char_p, P]
    L.cdc_files_clone.restype = ctypes.c_int64
    L.cdc_files_diff_device.argtypes = [P, P, ctypes.c_uint32, P, sz, ctypes.POINTER(cdc_diff_stats_t), P]
    L.cdc_files_diff_device.restype = ctypes.c_int64
    L.cdc_files_delta_device.argtypes = [P, P, ctypes.c_uint32, P, sz, ctypes.POINTER(cdc_delta_stats_t), P]
    L.cdc_files_delta_device.restype = ctypes.c_int64
    L.cdc_file_pack_device.argtypes = [P, P, P, P, sz, ctypes.POINTER(cdc_pack_stats_t), P]
    L.cdc_file_pack_device.restype = ctypes.c_int64
    L.cdc_files_unpack_device.argtypes = [P, ctypes.c_char_p, P, sz, P, ctypes.c_uint32,
                                          ctypes.POINTER(cdc_pack_stats_t), P]
    L.cdc_files_unpack_device.restype = ctypes.c_int64
    L.cdc_debug_splice_split.argtypes = [ctypes.POINTER(ctypes.c_double), sz]
    L.cdc_debug_splice_split.restype = ctypes.c_int
    L.cdc_debug_pack_split.argtypes = [ctypes.POINTER(ctypes.c_double), sz]
    L.cdc_debug_pack_split.restype = ctypes.c_int
    L.cdc_debug_file_slots.argtypes = [P, P, P, sz]
    L.cdc_debug_file_slots.restype = ctypes.c_int64
    L.cdc_fill_splitmix64_device.argtypes = [P, sz, ctypes.c_uint64, P]
    L.cdc_fill_splitmix64_device.restype = ctypes.c_int
    L.cdc_debug_pipeline.argtypes = [P]
    L.cdc_debug_pipeline.restype = ctypes.c_int
    L.cdc_debug_record_cap.argtypes = [P]
    L.cdc_debug_record_cap.restype = ctypes.c_uint32
    L.cdc_debug_read_bw.argtypes = [P, P, sz, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    L.cdc_debug_read_bw.restype = ctypes.c_int
    L.cdc_debug_host_placement.argtypes = [P, ctypes.c_char_p, sz]
    L.cdc_debug_host_placement.restype = ctypes.c_int64
    L.cdc_debug_copy.argtypes = [P, ctypes.c_int, P, sz]
    L.cdc_debug_copy.restype = ctypes.c_int64
    L.cdc_debug_files_table_blocks.argtypes = [P]
    L.cdc_debug_files_table_blocks.restype = ctypes.c_int64
    L.cdc_debug_collect_split.argtypes = [ctypes.POINTER(ctypes.c_double), sz]
    L.cdc_debug_collect_split.restype = ctypes.c_int
    L.cdc_version.argtypes = []
    L.cdc_version.restype = ctypes.c_char_p
    L.cdc_abi_version.argtypes = []
    L.cdc_abi_version.restype = ctypes.c_uint32
    del u8p
    _lib = L
    return L


def check(rc):
    """Raise CdcError for a negative return code, else return rc."""
    if rc < 0:
        raise CdcError(rc, lib().cdc_last_error().decode())
    return rc
