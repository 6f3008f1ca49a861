/*
 * chunkfs_amd_debug.h -- diagnostic entry points (not part of the drop-in
 * boundary).  They expose intermediate arrays of the LAST FastCDC batch of a
 * handle, so the scan's candidate records can be checked stage by stage on a
 * GPU (tests/test_gpu_resolve_paths.py).
 */
#ifndef CHUNKFS_AMD_DEBUG_H
#define CHUNKFS_AMD_DEBUG_H

#include "chunkfs_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* FastCDC pipeline of the handle: 3 (fastcdc.hip: scan + resolve), the only one. */
int cdc_debug_pipeline(const cdc_handle_t *h);
/* Candidate-record capacity per span (records are stored `cap` per span). */
uint32_t cdc_debug_record_cap(const cdc_handle_t *h);
/* Copy array `what` of the last batch to host memory `out` (at most
 * max_bytes): 0 = per-span candidate counts (u32; > cap means overflowed),
 * 1 = candidate records (u32, cap per span: offset in span (bits 0-23) |
 * truncated-region result of a chunk starting there (bits 24-29; 63 none, 62
 * not precomputed) | bit30 mask_l hit | bit31 mask_s hit).
 * When the handle's last FastCDC call (cdc_chunk_data, or a single-stream
 * cdc_chunk_batch_device) was taken by the one-launch kernel (small.hip) and
 * did not fall back, its scan stage can be read as well (CDC_EINVAL after any
 * other call): 2 = per-block record counts (u32, one per 32 KiB block of the
 * call; > 256 means the block overflowed), 3 = per-block record regions (u64,
 * 256 per block: bits 0-29 stream offset | bit30 mask_l hit | bit31 mask_s hit
 * | truncated-region result of a chunk starting there << 32 | that of its
 * max-cut successor << 40; 63 none, 62 left to the last block), 4 = the first
 * `len` bytes of the device copy of the input (a cdc_chunk_data call only:
 * CDC_EINVAL after a device-input call, which writes no copy).  5, 6, 7 = the
 * arrays of 2, 3, 4 at their full size (128 blocks, 4 MiB), i.e. with whatever
 * earlier calls left beyond the last call's blocks.
 * Returns the bytes copied or a negative CDC_E* code (CDC_EINVAL for any other
 * `what`). */
int64_t cdc_debug_copy(cdc_handle_t *h, int what, void *out, size_t max_bytes);
/* Host-path statistics into v[0..n): cdc_chunk_data calls, their upload
 * seconds (CPU copy into the pinned ring + queueing the H2D), their total
 * seconds, then the chunking seconds and segment count of the current or
 * last streaming write (cdc_write_*), then the FastCDC batches taken by the
 * one-launch small-stream kernel (small.hip) and how many of them fell back
 * to the regular pipeline (a record / start budget exceeded), then the
 * cdc_chunk_data calls whose chunk list did not tile the buffer when first
 * read and was read again after a stream synchronisation (expected 0). */
int cdc_debug_host_stats(const cdc_handle_t *h, double *v, size_t n);
/* Kernel times of the FastCDC batch `back` calls before the last one (0 = the
 * last; up to 63 back): scan_ms, resolve_ms, total_ms of t (the other fields
 * are the last batch's).  Each batch records its HIP events in its own slot of
 * a 64-entry ring, so a caller timing many back-to-back batches reads them
 * after the loop instead of waiting on each batch's events inside it.
 * Synchronous batches always record events; batches of
 * cdc_chunk_batch_device_async record them one in four
 * (CHUNKFS_AMD_EVENT_EVERY=k: one in k), the others report 0 ms.
 * CDC_EINVAL when that batch is not in the ring. */
int cdc_debug_timing_back(cdc_handle_t *h, uint32_t back, cdc_timing_t *t, size_t t_size);
/* Segment-walk handles (Rabin / UltraCDC / LeapCDC / SeqCDC / AE): what the
 * engine derived from the sizes at creation, into v[0..n), in this order:
 *   0 nbm         predicate bitmaps per segment (0 = byte mode)
 *   1 seg_log2    segments are 2^seg_log2 bytes
 *   2 warm        warm-up bytes before a segment
 *   3 cap         chunk starts recorded per segment
 *   4 piece_log2  the data-parallel passes run over 2^piece_log2-byte pieces
 *   5 rabin_mask  (1 << round(log2 avg)) - 1
 *   6 leap_thr    the CDC_LEAP_THRESHOLD entry in use
 * then, of the handle's last synchronous batch (0, 0 before one, and after
 * a batch with no bytes):
 *   7 its segment count
 *   8 how it ended: 0 = the fused end kernel and the gated output behind the
 *     first fix-up round, 1 = the gated output without the fused kernel, 2 =
 *     the ungated output after further rounds or the in-order pass.
 * Returns the number of values the library has (9; at most n are written), or
 * CDC_EINVAL for a FastCDC or fixed-size handle. */
int cdc_debug_walk_params(const cdc_handle_t *h, uint64_t *v, size_t n);
/* Measured-achievable HBM read rate on the handle's device: a read-only
 * reduction kernel (16-byte coalesced loads, every byte once) over the DEVICE
 * buffer d_buf[len], `reps` timed launches after one warm-up; *ms = the
 * average launch time (HIP events).  The denominator of the bench line's
 * roofline.frac_of_achievable. */
int cdc_debug_read_bw(cdc_handle_t *h, const uint8_t *d_buf, size_t len, int reps, double *ms);

/* Host placement of the boundary as a JSON object written into buf (cap bytes,
 * NUL-terminated, truncated if short): the device's PCI address, NUMA node
 * ("gpu_node", -1 unknown) and PCIe link (current and max), whether the pinned
 * ring / chunk list / staging were allocated on that node and the copy helpers
 * bound to its CPUs ("numa_placement"; CHUNKFS_AMD_COPY_NUMA=0 turns it off),
 * the node the ring and chunk list actually landed on, the CPUs this process
 * may use and how many of the helpers were pinned.  Allocates the ring if the
 * handle has none yet.  Returns the JSON length or a negative CDC_E* code. */
int64_t cdc_debug_host_placement(cdc_handle_t *h, char *buf, size_t cap);

/* Device blocks the file layer's span-table pool holds.  Span tables are carved
 * out of these blocks (a free list per capacity class, capacities doubling from
 * 64 spans), so a new file costs no device allocation; the blocks are released
 * by cdc_files_destroy.  CDC_EINVAL for a NULL layer. */
int64_t cdc_debug_files_table_blocks(const cdc_files_t *fs);

/* Where the last successful cdc_files_collect / cdc_store_retain_device of this
 * thread spent its time: wall milliseconds between the call's host waits (every
 * pass ends in one, so each figure covers the device work queued before it):
 * [0] references and survivor flags, [1] scratch and second-table allocation,
 * [2] survivor list, sort, new offsets and move plan, [3] index rebuild, [4] the
 * move, [5] table rewrite (0 for cdc_store_retain_device).  Copies min(n, 6)
 * entries and returns 6; CDC_EINVAL for n > 0 with NULL ms. */
int cdc_debug_collect_split(double *ms, size_t n);

/* The same for the last successful cdc_file_splice_device of this thread, all
 * rounds together: [0] the span search and the window read (the range planner and
 * the copy of the inserted bytes), [1] chunking, [2] resync, [3] SHA-256 and the
 * put, [4] the table build.  Copies min(n, 5) entries and returns 5; CDC_EINVAL
 * for n > 0 with NULL ms. */
int cdc_debug_splice_split(double *ms, size_t n);

/* The same for the last successful cdc_file_pack_device and the last successful
 * cdc_files_unpack_device of this thread.  Pack: [0] mark, flags and the two
 * scans, up to the wait for the sizes, [1] the header-and-sections kernel and the
 * copy of the data.  Unpack: [2] the header's way to the host, [3] the validation
 * kernel and the lookup, [4] the gather, SHA-256 and the comparison (the gather
 * alone with CDC_UNPACK_TRUST), [5] the put, [6] slots and the table build.
 * Copies min(n, 7) entries and returns 7; CDC_EINVAL for n > 0 with NULL ms. */
int cdc_debug_pack_split(double *ms, size_t n);

/* What a file's span table holds besides the offsets and digests the reads
 * return: per span the store's table slot and the arena offset resolved when the
 * span was written (HOST arrays of cap entries, either nullable).  Returns the
 * span count; a return > cap means nothing was written. */
int64_t cdc_debug_file_slots(cdc_fh_t *fh, uint32_t *slots, uint64_t *locs, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* CHUNKFS_AMD_DEBUG_H */
