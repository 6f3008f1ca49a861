/*
 * chunkfs_amd.h -- C ABI of the MI355X content-defined-chunking engine.
 *
 * This is the drop-in boundary for chunkfs's chunking hot path,
 * `Chunker::chunk_data` (reference src/lib.rs:74-86).  Every entry point below
 * names the reference item it replaces.  The signatures use plain pointers and
 * sizes only, so a Rust `impl Chunker`, ctypes or any other FFI
 * can bind them.
 *
 * Threading: one handle is NOT thread-safe (the reference serialises all calls
 * through ChunkerRef = Arc<Mutex<dyn Chunker>>, src/lib.rs:89-90).  Different
 * handles may be used concurrently, e.g. one per GPU.
 *
 * Errors: the reference's signatures are infallible and panic on bad sizes
 * (fastcdc's size assert!s).  Here every call returns CDC_OK / a count >= 0,
 * or a negative CDC_E* code, with a message from cdc_last_error().
 */
#ifndef CHUNKFS_AMD_H
#define CHUNKFS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: cdc_last_timing takes the caller's sizeof(cdc_timing_t) (the struct
 *    may grow; fields are only ever appended); cdc_abi_version().
 * 3: cdc_timing_t.path / .timed appended; cdc_chunk_batch_device_async,
 *    cdc_batch_sync.
 * 4: cdc_sha256_batch_device.
 * 5: cdc_store_* (device chunk store), CDC_ENOTFOUND.
 * 6: cdc_files_* / cdc_file_* (device file layer), CDC_EEXIST, CDC_EPERM.
 *    Added since, with no change to an existing entry point or struct (the
 *    number stays 6): the scrub stage -- cdc_store_set_target,
 *    cdc_store_scrub, cdc_store_scrub_stats, cdc_store_iterate_device,
 *    cdc_store_keys_device, cdc_scrub_measurements_t, cdc_scrub_stats_t,
 *    CDC_SCRUB_*; the bench fixture -- cdc_files_get_to_dedup_ratio,
 *    cdc_file_verify_device, cdc_store_size_distribution_device; the AE
 *    chunker -- CDC_ALGO_AE, cdc_create_ae; the batch write --
 *    cdc_files_write_batch_device, cdc_fwrite_t; removal and collection --
 *    cdc_files_remove, cdc_files_collect, cdc_store_retain_device,
 *    cdc_collect_stats_t; the edit in place -- cdc_file_splice_device,
 *    cdc_splice_stats_t; snapshots and diffs -- cdc_files_clone,
 *    cdc_files_diff_device, cdc_diff_stats_t, CDC_DIFF_TABLES_ONLY; packs --
 *    cdc_file_pack_device, cdc_files_unpack_device, cdc_pack_stats_t,
 *    CDC_UNPACK_TRUST; the second hasher -- CDC_HASH_SHA256,
 *    CDC_HASH_BLAKE2SP, cdc_hash_batch_device, cdc_store_set_hash,
 *    cdc_store_hash; the content-aligned delta -- cdc_files_delta_device,
 *    cdc_delta_op_t, cdc_delta_stats_t, CDC_DELTA_LITERAL,
 *    CDC_DELTA_TABLES_ONLY. */
#define CHUNKFS_AMD_ABI_VERSION 6

/* Chunk{offset,length} -- reference src/lib.rs:43-47 (usize fields; u64 here). */
typedef struct cdc_chunk {
    uint64_t offset;
    uint64_t length;
} cdc_chunk_t;

/* Algorithms of reference src/chunkers/mod.rs:3-9. */
typedef enum cdc_algo {
    CDC_ALGO_FASTCDC = 0, /* FastChunker  (src/chunkers/fast.rs)        */
    CDC_ALGO_FIXED = 1,   /* FSChunker    (src/chunkers/fixed_size.rs)  */
    CDC_ALGO_RABIN = 2,   /* RabinChunker (src/chunkers/rabin.rs)    -- parity unpinned */
    CDC_ALGO_SUPER = 3,   /* SuperChunker (src/chunkers/supercdc.rs) -- CDC_ENOTSUP */
    CDC_ALGO_ULTRA = 4,   /* UltraChunker (src/chunkers/ultra.rs)    -- parity unpinned */
    CDC_ALGO_LEAP = 5,    /* LeapChunker  (src/chunkers/leap.rs)     -- leap structure of the paper,
                             stand-in eligibility function (chunkfs_amd_cdc_params.h) */
    CDC_ALGO_SEQ = 6,     /* SeqChunker   (src/chunkers/seq.rs)      -- parity unpinned */
    CDC_ALGO_AE = 7       /* AE, asymmetric extremum (not in the reference: this project's
                             restatement of the published rule, DESIGN.md "AE") */
} cdc_algo_t;

#define CDC_OK 0
#define CDC_EINVAL (-1)  /* bad sizes / arguments (reference: fastcdc assert! panic) */
#define CDC_ENOMEM (-2)  /* device or host allocation failed */
#define CDC_EDEVICE (-3) /* HIP runtime error, or no usable gfx950 device */
#define CDC_ENOTSUP (-4) /* algorithm not implemented */
#define CDC_ENOTFOUND (-5) /* a requested digest is not in the store (reference: ErrorKind::NotFound) */
#define CDC_EEXIST (-6)  /* the file name is taken (reference: ErrorKind::AlreadyExists) */
#define CDC_EPERM (-7)   /* write through a read-only handle (reference: ErrorKind::PermissionDenied) */

typedef struct cdc_handle cdc_handle_t;

/* Create a chunker bound to one GPU.
 *   CDC_ALGO_FASTCDC: FastChunker::new(SizeParams{min,avg,max}) (fast.rs:11-15);
 *                     v2020 FastCDC, Level1 normalization (fast.rs:37).
 *                     Sizes: min 64..1 MiB, avg 256..4 MiB, max 1 KiB..16 MiB
 *                     (the crate's asserts), and max >= min and max >= avg:
 *                     below either the rule has no defined answer (max < min
 *                     cuts more chunks than cdc_max_chunk_count promises),
 *                     so such sizes are CDC_EINVAL.  min > avg, min == max
 *                     and avg == max are valid.
 *   CDC_ALGO_FIXED:   FSChunker::new(min) (fixed_size.rs:19-23); avg/max ignored.
 *   CDC_ALGO_RABIN / _ULTRA / _LEAP: RabinChunker / UltraChunker / LeapChunker
 *                     ::new(SizeParams{min,avg,max}) (rabin.rs:13-20,
 *                     ultra.rs:12-16, leap.rs:12-16).  The reference's crate
 *                     (cdc-chunkers 0.1.3) is absent: Rabin / Ultra restate the
 *                     published algorithms, parity unpinned; Leap
 *                     keeps the paper's leap structure with a STAND-IN window
 *                     eligibility function (not the published one).
 *                     Sizes: 0 < min <= avg <= max; Ultra min >= 8, Leap min >= 32.
 *   CDC_ALGO_SEQ:     SeqChunker with OperationMode::Increasing and the default
 *                     Config (cdc_create_seq for the full constructor).
 *   CDC_ALGO_AE:      AE in Max mode with the default window (cdc_create_ae
 *                     for the full constructor).
 *   CDC_ALGO_SUPER:   CDC_ENOTSUP.
 * Returns CDC_OK and *out, or a negative code. */
int cdc_create(cdc_algo_t algo, uint32_t min, uint32_t avg, uint32_t max,
               int device, cdc_handle_t **out);

/* SeqChunker::new(mode, sizes, config) (seq.rs:16-24): mode 0 = Increasing,
 * 1 = Decreasing; config = seq_length (pairs in the mode's direction that
 * end a chunk), jump_trigger (opposing pairs before a jump), jump_size
 * (bytes skipped); defaults 5 / 50 / 256 (include/chunkfs_amd_cdc_params.h). */
int cdc_create_seq(uint32_t mode, uint32_t seq_length, uint32_t jump_trigger,
                   uint32_t jump_size, uint32_t min, uint32_t avg, uint32_t max,
                   int device, cdc_handle_t **out);

/* AE, the asymmetric extremum chunker (Zhang et al., INFOCOM 2015), restated
 * by this project (parity with any crate unpinned).  v(i) is the big-endian
 * 32-bit value of the bytes i .. i+3, bytes at or past the end of the buffer of
 * the call (in a device batch: of the stream) reading 0; "better" is > in Max
 * mode (mode 0) and < in Min mode (mode 1).  A chunk starting at s with n
 * bytes left: n <= min ends it at n; otherwise, with L = min(n, max) and M
 * starting at s + (min > window + 1 ? min - (window + 1) : 0), positions i =
 * M+1 .. s+L-1 in order either move M to i (v(i) strictly better than v(M)) or,
 * at i == M + window, cut after i; no such i: the chunk is L long.
 * window == 0 takes the default, max(1, avg * 100000 / 171828)
 * (cdc_ae_default_window in chunkfs_amd_cdc_params.h: avg = (e - 1) window).
 * CDC_EINVAL unless 0 < min <= avg <= max, window + 1 <= max and mode <= 1.
 * The zero padding makes the last three values of a buffer depend on where it
 * ends: the streaming write path (1 MiB segments, each its own buffer) follows
 * the reference's StorageWriter loop over this rule and is NOT claimed equal
 * to one cdc_chunk_data over the whole write. */
int cdc_create_ae(uint32_t mode, uint32_t window, uint32_t min, uint32_t avg,
                  uint32_t max, int device, cdc_handle_t **out);

/* Drop(Chunker). */
void cdc_destroy(cdc_handle_t *h);

/* Chunker::chunk_data(&mut self, data: &[u8], empty: Vec<Chunk>) -> Vec<Chunk>
 * (src/lib.rs:80).  `data` is HOST memory (borrowed for the call, any alignment,
 * len may be 0).  Writes min(count, cap) chunks to `out` and returns the full
 * chunk count (snprintf convention: a return > cap means `out` was too small;
 * cdc_max_chunk_count() is always enough), or a negative CDC_E* code.
 * The chunks tile [0, len) exactly, in order. */
int64_t cdc_chunk_data(cdc_handle_t *h, const uint8_t *data, size_t len,
                       cdc_chunk_t *out, size_t cap);

/* Chunker::estimate_chunk_count (src/lib.rs:85): the reference's own formula,
 * len/min for FastCDC (fast.rs:47-49), Rabin, Ultra, Leap (rabin.rs:53-55,
 * ultra.rs:41-43, leap.rs:41-43), len/avg for Seq (seq.rs:52-54), len/size + 1
 * for fixed (fixed_size.rs:45-47). */
size_t cdc_estimate_chunk_count(const cdc_handle_t *h, size_t len);

/* A strict upper bound on the chunk count of `len` bytes (len/min + 1). */
size_t cdc_max_chunk_count(const cdc_handle_t *h, size_t len);

/* impl Debug for the chunker (fast.rs:52-56, fixed_size.rs:12-16), with the
 * engine suffix, e.g. "FastCDC (2020), sizes: SizeParams { min: 4096, avg:
 * 8192, max: 16384 } [MI355X gfx950]".  Owned by the handle. */
const char *cdc_describe(const cdc_handle_t *h);

/* Message for the last failing call on this thread ("" if none). */
const char *cdc_last_error(void);

/* Install a 256-entry GEAR table (fastcdc v2020 `GEAR`) for FastCDC handles.
 * The built-in table is a placeholder (include/chunkfs_amd_tables.h); a
 * maintainer pins parity with the Rust crate by passing the crate's table.
 * CDC_EINVAL while a streaming write (cdc_write_begin) is in progress on the
 * handle: one write never mixes two tables. */
int cdc_set_gear(cdc_handle_t *h, const uint64_t gear[256]);

/* Install the Rabin polynomial of a CDC_ALGO_RABIN handle (the reference's
 * RabinChunker carries its ChunkerParams tables, rabin.rs:34-51; the crate's
 * polynomial is absent offline, include/chunkfs_amd_cdc_params.h holds a
 * stand-in).  Degree 9..56 (the 48-byte window digest shifted by a byte stays
 * inside 64 bits); the tables are rebuilt for the handle.  CDC_EINVAL for
 * another algorithm or degree, and while a streaming write is in progress on
 * the handle (one write never mixes two polynomials). */
int cdc_set_rabin_poly(cdc_handle_t *h, uint64_t poly);

/* ---- Device-resident batch API (configs 2, 4, 5: inputs already in HBM) --
 * Chunk n independent streams in one pass.  d_streams[i] are DEVICE pointers
 * (16-byte aligned), lens[i] their byte lengths (host arrays of n entries).
 * The chunks of all streams are written to the DEVICE array d_out (offsets
 * relative to each stream's start), stream i occupying
 * d_out[first[i] .. first[i+1]); `first` is a HOST array of n+1 entries filled
 * by the call.  out_cap must be >= cdc_batch_max_chunks().  hip_stream is a
 * hipStream_t (NULL = the handle's own stream); the call returns after the
 * chunks are final (it synchronises that stream).  Returns the total chunk
 * count or a negative code.  No collective: multi-GPU runs give each rank its
 * own handle and its own streams (weak scaling). */
int64_t cdc_chunk_batch_device(cdc_handle_t *h, size_t n,
                               const uint8_t *const *d_streams,
                               const uint64_t *lens, cdc_chunk_t *d_out,
                               size_t out_cap, uint64_t *first,
                               void *hip_stream);

/* The same batch, enqueued: returns 0 once the batch is submitted, and
 * `first` (kept by the library until then) is filled by cdc_batch_sync.
 * FastCDC batches of more than 8 MiB are enqueued back to back with no host
 * round trip between them, their results collected later: the scans on
 * hip_stream, each resolve on a second stream of the handle behind its scan,
 * beside the next scan (CHUNKFS_AMD_OVERLAP=0 keeps both on hip_stream);
 * cdc_batch_sync orders hip_stream after the resolves.
 * Ordering, every algorithm: the batch reads d_streams' bytes after all work
 * enqueued on hip_stream (NULL: the handle's own stream) before this call --
 * input written by kernels or copies on hip_stream needs no host wait before
 * the submit.  FastCDC's scans run on hip_stream itself; a Rabin / Ultra /
 * Leap / Seq batch runs on a context's stream, which waits for an event
 * recorded on hip_stream at the submit.  Work on other streams is the
 * caller's to order.  d_streams' bytes and d_out must stay untouched from the
 * submit until cdc_batch_sync (work enqueued on hip_stream after the submit is
 * ordered after a FastCDC batch's scan only, and after nothing of a walk
 * batch).
 * Consecutive async batches of one handle must use one hip_stream (another
 * stream first completes the batches in flight).  Rabin / Ultra / Leap / Seq
 * batches of more than 8 MiB alternate between two internal contexts of the
 * handle (own streams, own host worker threads), so one batch's walks run
 * beside the next one's bitmap pass; they are complete (host-synchronised)
 * when cdc_batch_sync returns (CHUNKFS_AMD_WALK_ASYNC=0: inside this call).
 * Smaller batches and FSChunker complete inside this call (first filled on
 * return).
 * Any other call on the handle first completes the batches in flight. */
int64_t cdc_chunk_batch_device_async(cdc_handle_t *h, size_t n,
                                     const uint8_t *const *d_streams,
                                     const uint64_t *lens, cdc_chunk_t *d_out,
                                     size_t out_cap, uint64_t *first,
                                     void *hip_stream);

/* Completes every batch enqueued by cdc_chunk_batch_device_async (their
 * first[] arrays are filled); returns the last batch's total chunk count (0
 * when none was in flight) or a negative code. */
int64_t cdc_batch_sync(cdc_handle_t *h);

size_t cdc_batch_max_chunks(const cdc_handle_t *h, size_t n,
                            const uint64_t *lens);

/* Per-phase device time of the last batch (HIP events on the launch
 * stream), milliseconds.  scan = the gear candidate scan kernel (the HBM-bound
 * kernel the roofline is quoted on); resolve = truncated-region precompute +
 * the single-pass resolve (chain walk, look-back, output); compact = 0 (fused
 * into resolve); total = all of it. */
typedef struct cdc_timing {
    double scan_ms;
    double resolve_ms;
    double compact_ms;
    double total_ms;
    uint32_t fixup_iterations; /* spans whose speculative chain was re-walked */
    uint32_t overflow_spans; /* spans whose candidate list overflowed */
    uint64_t candidates;     /* candidate positions emitted by the scan */
    uint64_t bytes;          /* input bytes of the batch */
    double hash_ms;          /* last cdc_sha256_chunks_device / _batch_device / cdc_chunk_and_hash kernel time */
    uint64_t walk_fallback_steps; /* chain-walk steps without a precomputed record link */
    uint32_t path;           /* CDC_PATH_*: which engine path ran the batch */
    uint32_t timed;          /* 1: the *_ms fields were measured (HIP events); 0: not timed */
} cdc_timing_t;

/* cdc_timing_t.path */
#define CDC_PATH_PIPELINE 0 /* FastCDC scan + resolve */
#define CDC_PATH_SMALL 1    /* FastCDC one-launch small-stream kernel (not timed: no events on its call path) */
#define CDC_PATH_WALK 2     /* Rabin / Ultra / Leap / Seq segment-walk engine */
#define CDC_PATH_FIXED 3    /* FSChunker */
#define CDC_PATH_EMPTY 4    /* a batch of no streams */

/* Kernel times (HIP events) of the last batch; a batch enqueued by
 * cdc_chunk_batch_device_async carries events one in four (0 ms otherwise).
 * Copies min(t_size, sizeof(cdc_timing_t)) bytes: pass sizeof(cdc_timing_t)
 * of the header the caller was built with, so an older (shorter) struct is
 * never overrun when fields are appended in a later version. */
int cdc_last_timing(const cdc_handle_t *h, cdc_timing_t *t, size_t t_size);

/* ---- Write path ---------------------------------------
 * ChunkStorage::write (storage.rs:78-103) + StorageWriter::{write,flush}
 * (storage.rs:302-383) for ONE write call: seg_size slices (1 MiB in the
 * reference), carry-over of the last chunk of every segment, flush of the
 * rest.  Writes the span lengths in file order (min(count, cap) of them) and
 * returns the span count.  Runs the streaming path below with seg_size
 * segments.  *chunk_seconds (may be NULL) receives the wall time of the whole
 * call (host copy into pinned memory + H2D + chunking + chunk list), i.e. NOT
 * the reference's summed chunk_data time (storage.rs:314-316), which excludes
 * the copies: compare it with the reference's write time. */
int64_t cdc_fs_write(cdc_handle_t *h, const uint8_t *data, size_t len,
                     size_t seg_size, uint64_t *span_lengths, size_t cap,
                     double *chunk_seconds);

/* Streaming form of the same write (ChunkStorage::write_from_stream,
 * storage.rs:105-137: segments of any size, short reads included): begin,
 * then one cdc_write_segment per StorageWriter::write, then finish (=
 * StorageWriter::flush) returns the spans exactly as the reference's loop over
 * the same segments would.  A segment is copied into a handle-owned pinned
 * ring and uploaded asynchronously while the caller goes on; the device
 * chunks 256 MiB windows of the file, carrying each window's last chunk to the
 * next one in HBM.  The caller's bytes are not retained after a call returns.
 * One write per handle at a time: cdc_write_begin on a handle whose write is
 * in progress returns CDC_EINVAL.  A failing cdc_write_segment marks the write
 * failed: later segments return CDC_EINVAL and cdc_write_finish returns an
 * error (never spans of unknown correctness) and ends the write. */
int cdc_write_begin(cdc_handle_t *h);
int cdc_write_segment(cdc_handle_t *h, const uint8_t *data, size_t len);
/* Spans that became final since the last drain, oldest first: moves
 * min(pending, cap) of them into span_lengths and returns how many it moved
 * (0: none pending).  Spans become final each time a device window has been
 * chunked, i.e. every 256 MiB of uploaded bytes, so a caller that hashes and
 * stores each span as StorageWriter::write does (storage.rs:324-350) needs to
 * keep only the bytes from the end of the last drained span on: at most one
 * window (256 MiB) + the segment in hand + max bytes, as the reference's
 * write_from_stream keeps SEG_SIZE + max. */
int64_t cdc_write_drain(cdc_handle_t *h, uint64_t *span_lengths, size_t cap);
/* The spans no cdc_write_drain returned (min(count, cap) written), returns
 * their count; *seconds (may be NULL) = wall time since cdc_write_begin. */
int64_t cdc_write_finish(cdc_handle_t *h, uint64_t *span_lengths, size_t cap,
                         double *seconds);

/* ---- Chunk fingerprints -------------------------------
 * Sha256Hasher::hash (src/hashers.rs:20-36), applied to every chunk as
 * StorageWriter::write does (storage.rs:324-329).  DEVICE arrays:
 * d_digests[32*i .. 32*i+32) = SHA-256(d_data[d_chunks[i].offset .. +length)).
 * Synchronises hip_stream (NULL = the handle's stream) before returning. */
int cdc_sha256_chunks_device(cdc_handle_t *h, const uint8_t *d_data,
                             const cdc_chunk_t *d_chunks, size_t n_chunks,
                             uint8_t *d_digests, void *hip_stream);

/* The same over a batch of streams in one launch -- e.g. the output of
 * cdc_chunk_batch_device: stream i's chunks are d_chunks[first[i] ..
 * first[i+1]) with offsets relative to d_streams[i]; first[0] must be 0.
 * d_streams (n_streams device pointers, 4-byte aligned) and first
 * (n_streams + 1 entries) are HOST arrays; d_chunks / d_digests are DEVICE
 * arrays of first[n_streams] entries (32-byte digests, chunk order).  Each
 * stream's chunks must lie inside its buffer.  Synchronises hip_stream. */
int cdc_sha256_batch_device(cdc_handle_t *h, size_t n_streams,
                            const uint8_t *const *d_streams, const uint64_t *first,
                            const cdc_chunk_t *d_chunks, uint8_t *d_digests,
                            void *hip_stream);

/* The chunk hashers (the reference is generic over its Hasher trait,
 * src/hashers.rs).  Both give 32-byte digests, so every table, index key and
 * pack section has one layout.  CDC_HASH_BLAKE2SP is unkeyed BLAKE2sp-256
 * (8 BLAKE2s leaves and a root: DESIGN.md "Hashers"), digest bytes in
 * BLAKE2's own order. */
#define CDC_HASH_SHA256 0
#define CDC_HASH_BLAKE2SP 1

/* cdc_sha256_batch_device with the hasher as an argument: the same arrays,
 * validation, refusals and hash_ms.  An unknown `hash` is CDC_EINVAL.
 * cdc_sha256_batch_device is this call with CDC_HASH_SHA256. */
int cdc_hash_batch_device(cdc_handle_t *h, int hash, size_t n_streams,
                          const uint8_t *const *d_streams, const uint64_t *first,
                          const cdc_chunk_t *d_chunks, uint8_t *d_digests, void *hip_stream);

/* chunk_data + SHA-256 of each chunk on a HOST buffer: as cdc_chunk_data, and
 * digests[32*i ..] for the first min(count, cap) chunks. */
int64_t cdc_chunk_and_hash(cdc_handle_t *h, const uint8_t *data, size_t len,
                           cdc_chunk_t *out, uint8_t *digests, size_t cap);

/* ---- Dedup index --------------------------------------
 * The chunk Database of the reference keyed by SHA-256 digest
 * (src/system/database.rs:74-87: HashMap, `entry(key).or_insert`, i.e. the
 * FIRST insert of a digest wins) and the storage statistics built on it
 * (src/system/storage.rs:193-240), as a device hash set. */
typedef struct cdc_index cdc_index_t;

typedef struct cdc_index_stats {
    uint64_t chunks_written;  /* chunks inserted so far */
    uint64_t bytes_written;   /* size_written: bytes of all inserted chunks */
    uint64_t unique_chunks;   /* distinct digests */
    uint64_t unique_bytes;    /* total_cdc_size: bytes of the first chunk of each digest */
} cdc_index_stats_t;
/* cdc_dedup_ratio = bytes_written / unique_bytes (storage.rs:203-205);
 * average_chunk_size = unique_bytes / unique_chunks (storage.rs:208-220). */

/* Index on `device` for up to `capacity` distinct digests. */
int cdc_index_create(int device, size_t capacity, cdc_index_t **out);
void cdc_index_destroy(cdc_index_t *ix);
/* Database::clear + size_written = 0 (storage.rs:236-240). */
int cdc_index_clear(cdc_index_t *ix);
/* Database::insert of n (digest, chunk) pairs in chunk order (DEVICE arrays:
 * 32-byte digests, cdc_chunk_t records).  d_new (nullable, DEVICE u8[n])
 * receives 1 where the chunk's digest was not in the index before it.
 * Returns the number of new digests (CDC_ENOMEM past capacity). */
int64_t cdc_index_insert_device(cdc_index_t *ix, const uint8_t *d_digests,
                                const cdc_chunk_t *d_chunks, size_t n,
                                uint8_t *d_new, void *hip_stream);
int cdc_index_stats(const cdc_index_t *ix, cdc_index_stats_t *out);

/* ---- Chunk store ----------------------------------------------------------------
 * The reference's key -> data Database (src/system/database.rs:10-36, 74-87:
 * insert / get / get_multi / contains, the FIRST insert of a key wins),
 * ChunkStorage::retrieve (src/system/storage.rs:141-157) and
 * FileSystem::read_file_complete / read_from_file (src/system/mod.rs:149-160:
 * look up every span's hash, concatenate), on one GPU: a dedup index as above
 * plus an HBM arena that holds the bytes of each first-seen chunk.
 *
 * Stream ordering: every call runs on hip_stream (NULL = the store's own
 * non-blocking stream) and synchronises it before returning, as
 * cdc_index_insert_device does.  Input written by earlier work on hip_stream
 * needs no host wait.  One store is NOT thread-safe; different stores may be
 * used concurrently.
 *
 * A refused call changes nothing.  put first runs a small kernel over the chunk
 * list and checks on the host, before it touches the table or the arena:
 *   every chunk lies inside its buffer (offset + length <= data_len / lens[i],
 *     computed without overflow), else CDC_EINVAL;
 *   unique_chunks + n <= max_chunks, else CDC_ENOMEM;
 *   arena_used + sum of round_up(length, 16) over ALL n chunks <= arena_capacity,
 *     else CDC_ENOMEM
 * -- "as if every chunk were new", the index's own rule.  After a refused put,
 * get or contains the stats equal those before and every stored digest is
 * still retrievable.  Result-dependent errors are the index's: a full table or
 * too many 64-bit key collisions return its error (CDC_ENOMEM).
 *
 * Lookup compares the full 32-byte digest and goes on probing past a slot whose
 * 64-bit key matches but whose digest differs (the index places such a digest
 * further along the probe sequence); it stops at an empty slot or after
 * `slots` probes.
 *
 * Arena layout: stored chunks start at 16-byte multiples.  The new chunks of a
 * put are laid out in chunk order -- an exclusive scan of the padded lengths
 * over the `new` flags, starting at arena_used -- so the layout is
 * deterministic.  Padding bytes are unspecified.  Length-0 chunks are legal:
 * stored with no bytes, returned as an empty span.  Offsets and lengths are 64
 * bits throughout. */
typedef struct cdc_store cdc_store_t;

typedef struct cdc_store_stats {
    cdc_index_stats_t index;  /* same meaning as cdc_index_stats */
    uint64_t arena_capacity;  /* bytes */
    uint64_t arena_used;      /* bytes, including the 16-byte padding of each stored chunk */
} cdc_store_stats_t;

/* Store on `device` for up to max_chunks distinct digests and arena_bytes of
 * chunk data (neither grows later). */
int cdc_store_create(int device, size_t max_chunks, size_t arena_bytes, cdc_store_t **out);
void cdc_store_destroy(cdc_store_t *st);
/* clear_database (storage.rs:236-240): empties the table, arena_used = 0. */
int cdc_store_clear(cdc_store_t *st);
int cdc_store_stats(const cdc_store_t *st, cdc_store_stats_t *out);

/* Database::insert of n (digest, chunk bytes) pairs in chunk order; chunk i is
 * d_data[d_chunks[i].offset .. +length) (DEVICE arrays; d_data at any
 * alignment).  The first insert of a digest wins, within the batch and across
 * calls; only first occurrences are copied into the arena.  d_new (nullable,
 * DEVICE u8[n]) as in cdc_index_insert_device.  Returns the number of new
 * digests. */
int64_t cdc_store_put_device(cdc_store_t *st, const uint8_t *d_data, size_t data_len,
                             const cdc_chunk_t *d_chunks, const uint8_t *d_digests,
                             size_t n, uint8_t *d_new, void *hip_stream);

/* The same for the output of cdc_chunk_batch_device + cdc_sha256_batch_device:
 * d_streams / lens / first are HOST arrays (n_streams, n_streams, n_streams + 1
 * entries; first[0] = 0), chunk offsets relative to each stream, n =
 * first[n_streams].  Global chunk order = stream order. */
int64_t cdc_store_put_batch_device(cdc_store_t *st, size_t n_streams,
                                   const uint8_t *const *d_streams, const uint64_t *lens,
                                   const uint64_t *first, const cdc_chunk_t *d_chunks,
                                   const uint8_t *d_digests, uint8_t *d_new, void *hip_stream);

/* ChunkStorage::retrieve(...).concat() / Database::get_multi: the chunks of
 * d_digests[0..n) (DEVICE, 32 bytes each), in request order, back to back in
 * the DEVICE buffer d_out (any alignment).  d_spans (nullable, DEVICE
 * cdc_chunk_t[n]) receives each one's {offset in d_out, length}.  Returns the
 * total byte count (snprintf convention: a return > out_cap means NOTHING was
 * written to d_out or d_spans; out_cap = 0 sizes a read).  CDC_ENOTFOUND if
 * any digest is absent (nothing written). */
int64_t cdc_store_get_device(cdc_store_t *st, const uint8_t *d_digests, size_t n,
                             uint8_t *d_out, size_t out_cap, cdc_chunk_t *d_spans,
                             void *hip_stream);

/* Database::contains for n digests: d_found[i] (DEVICE u8[n]) = 1/0.  Returns
 * how many were found. */
int64_t cdc_store_contains_device(cdc_store_t *st, const uint8_t *d_digests, size_t n,
                                  uint8_t *d_found, void *hip_stream);

/* ---- Scrub stage -----------------------------------------------------------------
 * The reference's second stage: the Scrub hook (src/system/scrub.rs:31-64),
 * the DataContainer that is either a chunk or a list of target keys
 * (src/system/storage.rs:12-21), the target map, retrieve through target keys
 * (storage.rs:141-157), and new_with_scrubber / scrub / total_dedup_ratio /
 * storage_iterator / clear_file_system (src/system/mod.rs:226-298).
 *
 * The target map is a second cdc_store_t: its key is the 32-byte SHA-256 of the
 * value, a Database<Hash, Vec<u8>>.  The base store keeps, per slot, the
 * container's kind and -- for a target -- a run of resolved keys: the target
 * store's slot and the byte offset of the key's value inside the container.  A
 * read goes from slot to target location with no digest lookup.
 *
 * Once a store holds target-kind containers, cdc_store_get_device expands a
 * digest into the pieces of its keys (d_spans still reports one {offset,
 * length} per digest; every convention of the call is unchanged) and
 * cdc_store_contains_device is true for them.  The file layer finds a span's
 * bytes through its slot's current container.  Writes go on as before: a digest
 * that exists as a target adds nothing (first insert wins), a new digest
 * becomes a chunk-kind container.
 *
 * A COPY or RECHUNK scrub converts every chunk-kind container, so afterwards no
 * byte of the base arena is live: arena_used becomes 0 and later writes fill
 * the arena again from the start.
 *
 * A refused scrub changes nothing.  Before the target or the base is touched, a
 * planning pass computes the key count and the sum of round_up(length, 16) "as
 * if every key were new" (for RECHUNK by chunking every group once for the
 * counts; a scrub that fits one group keeps its lists and does not chunk
 * twice) and returns CDC_ENOMEM if the target's max_chunks or arena cannot take
 * that much.  The index's result-dependent errors (a table full of 64-bit key
 * collisions) stay what they are for put: they can leave the containers of
 * earlier groups converted, each still readable.
 *
 * Epochs: the base remembers the target's clear count.  After
 * cdc_store_clear(target), a read that needs a target-kind container returns
 * CDC_ENOTFOUND and writes nothing, and a scrub returns CDC_ENOTFOUND while
 * target-kind containers exist; cdc_store_clear(base) drops the containers and
 * keys, keeps the attachment and adopts the target's present state. */
#define CDC_SCRUB_DUMB 0    /* DumbScrubber (scrub.rs:116-129): does nothing, all-zero measurements */
#define CDC_SCRUB_COPY 1    /* CopyScrubber (scrub.rs:85-114): target.insert(hash, chunk), make_target([hash]) */
#define CDC_SCRUB_RECHUNK 2 /* this project's own, no counterpart in the reference: every chunk container is
                               chunked again with `chunker`, keys = SHA-256 of the sub-chunks, each
                               (key, sub-chunk) inserted into the target, make_target(keys).  A length-0
                               chunk becomes a target with no keys. */

/* ScrubMeasurements (scrub.rs:71-79). */
typedef struct cdc_scrub_measurements {
    uint64_t processed_data;  /* bytes of the chunk containers the scrubber converted */
    double running_seconds;   /* wall time of the call */
    uint64_t data_left;       /* 0: the provided scrubbers convert every chunk container or none */
} cdc_scrub_measurements_t;

typedef struct cdc_scrub_stats {
    uint64_t cdc_bytes;          /* total_cdc_size (storage.rs:193-200): bytes of the chunk-kind containers */
    uint64_t chunk_containers;
    uint64_t target_containers;
    uint64_t keys;               /* over all target-kind containers */
    uint64_t target_bytes;       /* sum of the target map's value lengths (storage.rs:250-257) */
    uint64_t target_values;
} cdc_scrub_stats_t;

/* ChunkStorage::new_with_scrubber's target_map (storage.rs:165-178): `target`
 * becomes the target map of `base` (not owned: destroy the base first).
 * CDC_EINVAL if either is NULL, base == target, they are on different devices,
 * `target` has a target itself, `base` holds target-kind containers, or the
 * two stores have different hashers (cdc_store_set_hash). */
int cdc_store_set_target(cdc_store_t *base, cdc_store_t *target);
/* The hasher of the store's digests (CDC_HASH_*; a new store: CDC_HASH_SHA256):
 * the file layer (single and batch write, splice, the unpack's integrity
 * check) and the RECHUNK scrub hash with it, and a pack carries it in its
 * header.  cdc_store_put_device takes digests as given: the caller hashes with
 * cdc_hash_batch_device(cdc_store_hash(st)).  Changing it is allowed only
 * while the store is empty and stands alone: CDC_EINVAL if the store holds a
 * chunk (after cdc_store_clear it is allowed again), a target store is
 * attached, the store has been made another store's target, or `hash` is
 * unknown. */
int cdc_store_set_hash(cdc_store_t *st, int hash);
int cdc_store_hash(const cdc_store_t *st);
/* ChunkStorage::scrub (storage.rs:180-190) with one of the CDC_SCRUB_*
 * scrubbers; CDC_EINVAL without a target ("scrubber cannot be used with CDC
 * filesystem").  `chunker` is used by RECHUNK only and must be on the store's
 * device; every algorithm is allowed.  RECHUNK works in groups of containers
 * (one cdc_chunk_batch_device + cdc_sha256_batch_device + put each) so that its
 * scratch stays bounded; CHUNKFS_AMD_SCRUB_GROUP=containers[,bytes] sets the
 * bounds of a group. */
int cdc_store_scrub(cdc_store_t *base, int scrubber, cdc_handle_t *chunker,
                    cdc_scrub_measurements_t *out, void *hip_stream);
/* The numbers behind cdc_dedup_ratio / average_chunk_size / full_cdc_dedup_ratio
 * (storage.rs:193-231) and total_dedup_ratio (storage.rs:250-261).  Without a
 * target: cdc_bytes = unique_bytes, the rest 0. */
int cdc_store_scrub_stats(const cdc_store_t *base, cdc_scrub_stats_t *out);
/* ChunkStorage::iterator (storage.rs:233-235, FileSystem::storage_iterator,
 * mod.rs:266-269): per occupied slot, in slot order, the digest (32 bytes), the
 * kind (0 chunk, 1 target), the length the container restores to, and
 * d_key_first[n + 1] -- container i owns keys [d_key_first[i], d_key_first[i +
 * 1]) of cdc_store_keys_device.  DEVICE arrays of cap (cap + 1) entries.
 * Returns n; a return > cap means nothing was written.  The order is
 * unspecified but the same for both calls while the store is not modified. */
int64_t cdc_store_iterate_device(cdc_store_t *st, uint8_t *d_digests, uint8_t *d_kinds,
                                 uint64_t *d_lengths, uint64_t *d_key_first, size_t cap,
                                 void *hip_stream);
/* The flat 32-byte keys of every target-kind container, in the same order.
 * Returns the key count; a return > cap means nothing was written. */
int64_t cdc_store_keys_device(cdc_store_t *st, uint8_t *d_keys, size_t cap, void *hip_stream);

/* ---- File layer ------------------------------------------------------------------
 * The reference's FileLayer (src/system/file_layer.rs) and the FileSystem calls
 * built on it (src/system/mod.rs:58-160, 271-278), bound to one chunk store:
 * named files, each the ordered span list {hash, offset, len}
 * (file_layer.rs:9-23).  Names and handles live on the host; each file's span
 * table lives in HBM (the n + 1 byte offsets, the 32-byte digests, and per span
 * the table slot and arena offset the store resolved when it was written), and
 * every per-span step runs on the GPU.  A read goes from span to bytes with no
 * digest lookup and no host check before the copy.
 *
 * Stream ordering and thread-safety are the store's: each call runs on
 * hip_stream (NULL = the store's own stream) and synchronises it once before
 * returning; one layer and its store are NOT thread-safe.  Calls on the bound
 * store may be mixed with calls on the layer.
 *
 * A refused call changes nothing: a write the store refuses (CDC_ENOMEM,
 * CDC_EINVAL) leaves the file's span count and size as they were; a read into
 * too small a buffer returns the size it needs and writes nothing (snprintf
 * convention, out_cap = 0 sizes a read).  If the bound store was cleared with
 * cdc_store_clear since a file's spans were written, reads of that file and
 * further writes to it return CDC_ENOTFOUND and write nothing.
 *
 * ONE deviation from the reference: a span's offset is always its true byte
 * position in the file.  The reference derives it from the handle
 * (file_layer.rs:136-145), and a handle from open starts at 0, so appending
 * through a re-opened handle restarts the offsets at 0 and read then skips
 * spans.  For a file written through one handle the two agree exactly, and
 * read_file_complete agrees always.
 *
 * Two quirks of the reference are reproduced: a first span longer than the
 * segment makes cdc_file_read_device return 0 with the cursor stuck
 * (file_layer.rs:160-167), and the distribution leaves out the file's last span
 * (file_layer.rs:193-197). */
typedef struct cdc_files cdc_files_t; /* the layer */
typedef struct cdc_fh cdc_fh_t;       /* FileHandle (file_layer.rs:32-41) */

typedef struct cdc_file_stat {
    uint64_t size;        /* bytes: the sum of the span lengths */
    uint64_t spans;
    uint64_t cursor;      /* FileHandle::offset as cdc_file_read_device advances it */
    double chunk_seconds; /* WriteMeasurements of this handle's cdc_file_write_device calls: */
    double hash_seconds;  /* wall time of the chunking and of the SHA-256 step, summed */
} cdc_file_stat_t;

/* One range of cdc_files_pread_batch_device. */
typedef struct cdc_pread {
    cdc_fh_t *fh;
    uint64_t offset;
    uint64_t len;
    uint8_t *d_dst; /* DEVICE, len bytes, any alignment */
} cdc_pread_t;

/* One file of cdc_files_write_batch_device. */
typedef struct cdc_fwrite {
    cdc_fh_t *fh;
    const uint8_t *d_data; /* DEVICE, 16-byte aligned when len > 0 */
    uint64_t len;
} cdc_fwrite_t;

/* FileLayer::default over `store` (not owned: destroy the layer first).
 * seg_size is the segment of cdc_file_read_device, SEG_SIZE of
 * file_layer.rs:162; 0 = 1 MiB. */
int cdc_files_create(cdc_store_t *store, size_t seg_size, cdc_files_t **out);
/* Open handles must still be closed with cdc_file_close; their other calls
 * return CDC_EINVAL from here on. */
void cdc_files_destroy(cdc_files_t *fs);
/* FileSystem::clear_database (mod.rs:275-278): FileLayer::clear
 * (file_layer.rs:183-185) and cdc_store_clear.  Every open handle is
 * invalidated: its calls return CDC_ENOTFOUND until a file of its name is
 * created again. */
int cdc_files_clear(cdc_files_t *fs);
/* FileLayer::file_exists (file_layer.rs:178-180): 1 / 0. */
int cdc_files_exists(const cdc_files_t *fs, const char *name);
/* FileLayer::list_files (file_layer.rs:271-273): the names in byte order, each
 * followed by a NUL.  Returns the bytes needed; a return > cap means nothing
 * was written. */
int64_t cdc_files_list(const cdc_files_t *fs, char *buf, size_t cap);

/* FileLayer::create (file_layer.rs:84-99): CDC_EEXIST if !create_new and the
 * name exists; otherwise creates the file or replaces it with an empty one
 * (FileSystem::create_file passes true, mod.rs:81-87).  The handle may write. */
int cdc_files_create_file(cdc_files_t *fs, const char *name, int create_new, cdc_fh_t **out);
/* FileLayer::open / open_readonly (file_layer.rs:102-114): CDC_ENOTFOUND for an
 * unknown name.  Several handles may be open on one file; every handle starts
 * with its cursor at 0. */
int cdc_files_open(cdc_files_t *fs, const char *name, int readonly, cdc_fh_t **out);
/* FileHandle::close (file_layer.rs:77-79); read the measurements with
 * cdc_file_stat first. */
void cdc_file_close(cdc_fh_t *fh);
int cdc_file_stat(cdc_fh_t *fh, cdc_file_stat_t *out);

/* FileSystem::write_to_file (mod.rs:93-110) for data already in HBM: one
 * chunk_data over the whole call (cdc_chunk_batch_device, one stream), SHA-256
 * of every chunk (cdc_sha256_batch_device), put into the store, spans appended
 * (file_layer.rs:136-148) -- in buffers the layer owns, nothing but the counts
 * crossing to the host.  d_data: DEVICE, 16-byte aligned (what FastCDC asks of
 * device streams).  Returns the number of spans appended; CDC_EPERM through a
 * read-only handle. */
int64_t cdc_file_write_device(cdc_fh_t *fh, cdc_handle_t *chunker, const uint8_t *d_data, size_t len,
                              void *hip_stream);
/* The same for callers that chunked and hashed already: arguments as
 * cdc_store_put_device.  Chunks need not tile the data; length-0 chunks are
 * legal.  A span's length is that of the chunk stored under its digest. */
int64_t cdc_file_append_device(cdc_fh_t *fh, const uint8_t *d_data, size_t data_len, const cdc_chunk_t *d_chunks,
                               const uint8_t *d_digests, size_t n, void *hip_stream);

/* n FileSystem::write_to_file calls (mod.rs:93-110) as one: every request is one
 * chunk_data over its whole buffer, as cdc_file_write_device -- but all requests
 * share one cdc_chunk_batch_device (each request a stream of its own: AE and
 * every other chunker see it as its own buffer), one cdc_sha256_batch_device,
 * one put and one segmented append, so the host waits for the device a fixed
 * number of times however many files there are.  reqs: HOST array of n entries.
 * Returns the total number of spans appended; spans (HOST[n], nullable)
 * receives each request's count.
 *
 * The contract: after the call everything observable equals n calls of
 * cdc_file_write_device in request order on the same starting state -- every
 * file's cdc_file_stat size and span count, its digest sequence, the span
 * offsets and the bytes read back, the distribution, and cdc_store_stats in
 * every field, arena_used included.  First insert wins in request order, and the
 * arena layout is the chunk-order layout of cdc_store_put_batch_device; in the
 * scrubbed state a digest that exists as a target adds nothing, as in a put.
 * Stream and epoch conventions are cdc_file_write_device's.  n == 0 returns 0;
 * a request with len == 0 is legal, appends nothing and reports 0 spans.
 *
 * All or nothing -- a refused call changes no file and not the store:
 *   CDC_EINVAL    a NULL argument, len > 0 with NULL data, a handle of another
 *                 layer or one that outlived its layer, two requests naming the
 *                 same file, or (from the put) a chunk outside its buffer;
 *   CDC_EPERM     a read-only handle anywhere in the list;
 *   CDC_ENOTFOUND an unknown file, or one whose spans predate a store clear;
 *   CDC_ENOMEM    the put's: max_chunks or the arena too small "as if every
 *                 chunk were new", over the whole batch.
 * Span tables may have grown in capacity before a refusal; their contents have
 * not changed.
 *
 * Each handle's chunk_seconds / hash_seconds grow by the batch's chunking /
 * hashing wall time times len_i / sum of len, so they sum to the batch's time. */
int64_t cdc_files_write_batch_device(cdc_files_t *fs, cdc_handle_t *chunker, size_t n, const cdc_fwrite_t *reqs,
                                     uint64_t *spans, void *hip_stream);

/* FileSystem::read_file_complete (mod.rs:149-152): every span in order, back to
 * back in d_out (DEVICE, any alignment); d_spans (nullable, DEVICE
 * cdc_chunk_t[spans]) receives each span's {offset, length}.  Returns the
 * file's size; a return > out_cap means nothing was written. */
int64_t cdc_file_read_complete_device(cdc_fh_t *fh, uint8_t *d_out, size_t out_cap, cdc_chunk_t *d_spans,
                                      void *hip_stream);
/* FileSystem::read_from_file (mod.rs:157-160, file_layer.rs:152-175): from the
 * handle's cursor, whole spans while their running total stays <= the layer's
 * segment size; the cursor advances by the bytes returned.  0 at the end of the
 * file, and 0 with the cursor unchanged when the span at the cursor is longer
 * than the segment (as in the reference).  A return > out_cap: nothing
 * written, cursor unchanged. */
int64_t cdc_file_read_device(cdc_fh_t *fh, uint8_t *d_out, size_t out_cap, void *hip_stream);
/* Not in the reference: the bytes [offset, min(offset + len, size)) of the file
 * into d_out (DEVICE, len bytes, any alignment).  Returns the count like
 * pread(2); len = 0 or offset >= size gives 0.  The cursor is not used. */
int64_t cdc_file_pread_device(cdc_fh_t *fh, uint64_t offset, size_t len, uint8_t *d_out, void *hip_stream);
/* n ranges over any files of the layer, planned and copied as one piece list.
 * reqs and got are HOST arrays of n entries; got[i] = bytes of request i.
 * Destinations must not overlap. */
int cdc_files_pread_batch_device(cdc_files_t *fs, size_t n, const cdc_pread_t *reqs, uint64_t *got,
                                 void *hip_stream);
/* FileLayer::read_complete (file_layer.rs:127-133): the spans' digests, in
 * order (DEVICE, 32 bytes each).  Returns the span count; a return > cap means
 * nothing was written.  Runs on the store's own stream. */
int64_t cdc_file_hashes_device(cdc_fh_t *fh, uint8_t *d_digests, size_t cap);

/* FileLayer::chunk_count_distribution (file_layer.rs:188-206) over spans
 * 0 .. n-2 (the reference's zip with skip(1) drops the last span): per distinct
 * digest its count and the length of its first occurrence, in order of first
 * occurrence in the file (the reference's map is unordered).  DEVICE arrays of
 * cap entries (32-byte digests, u32 counts, u64 lengths).  Returns the number
 * of distinct digests; a return > cap means nothing was written. */
int64_t cdc_file_distribution_device(cdc_fh_t *fh, uint8_t *d_digests, uint32_t *d_counts, uint64_t *d_lengths,
                                     size_t cap, void *hip_stream);

/* ---- Bench fixture ------------------------------------------------------------------
 * What the reference's CDCFixture (src/bench/mod.rs:66-283) needs beyond the
 * file system calls above, on what is already in HBM: a derived file with a
 * chosen dedup ratio, verification of a file against a dataset without reading
 * it back, and the chunk-size histogram of the store.  Stream, epoch and error
 * conventions are the file layer's and the store's.
 *
 * Three refusals the reference does not have: a NaN or infinite ratio (it would
 * produce an empty or unbounded file), repeating spans that are all empty (its
 * cycle would never end) and adjustment == 0 (it divides by zero). */

/* FileLayer::get_to_dedup_ratio (file_layer.rs:208-268; FileSystem, mod.rs:170-178):
 * a new file "{name}.{ratio:.2}" (printf "%.2f") made of the spans of file
 * `name`, so that its size is about dedup_ratio times its unique bytes.
 *   unique list: spans 0 .. n-2 of `name` (the last span is left out, as in
 *     cdc_file_distribution_device), the first occurrence of each digest in
 *     file order with its length: uniq[0..U), unique_length bytes in all;
 *   total_size = (uint64)((double)unique_length * ratio),
 *     R = (uint64)ceil((double)U * (1.0 / ratio)), in IEEE double as written there;
 *   repeating part: cycle over uniq[0..R), taking entries while the running byte
 *     sum stays <= total_size (entries of length 0 count): K spans;
 *   the new file has K + (U - R) spans: span i < K is uniq[i mod R], span
 *     i >= K is uniq[R + i - K].
 * It replaces any file of that name (HashMap::insert); open handles on the
 * replaced file see the new one.  The file layer's deviation applies: a span's
 * offset is its true byte position in the new file (the reference clones each
 * span with the offset it had in the source); read_file_complete and the digest
 * sequence agree with the reference exactly.  The new file shares the source's
 * store epoch and resolved locations, so it reads in the scrubbed state too.
 * A source of 0 or 1 spans gives an empty new file.
 * Returns the bytes the new name needs, its NUL included; a return > out_cap
 * means the name was NOT written -- the file was still created.
 * CDC_EINVAL: ratio < 1, NaN or infinite; R >= 1 while the first R unique spans
 * hold no byte.  CDC_ENOTFOUND: unknown name, or the store was cleared since
 * the source was written.  CDC_ENOMEM: the new span table cannot be allocated.
 * A refused call changes nothing. */
int64_t cdc_files_get_to_dedup_ratio(cdc_files_t *fs, const char *name, double dedup_ratio, char *out_name,
                                     size_t out_cap, void *hip_stream);

/* CDCFixture::verify (bench/mod.rs:241-275) without the read-back: 1 when the
 * file's bytes equal d_data[0..len) (DEVICE, any alignment), 0 otherwise.
 * *first_diff (HOST, nullable) receives the smallest differing byte offset,
 * min(size, len) when the common prefix is equal but the sizes differ, ~0 when
 * the two are equal.  The read planner's piece list feeds a compare kernel in
 * place of the copy: 2 bytes read and none written per file byte.  The call
 * never reads outside [d_data, d_data + len).  Epochs, stream and errors as
 * cdc_file_read_complete_device. */
int64_t cdc_file_verify_device(cdc_fh_t *fh, const uint8_t *d_data, size_t len, uint64_t *first_diff,
                               void *hip_stream);

/* CDCFixture::size_distribution (bench/mod.rs:218-232): over every occupied
 * slot of the store, the count per length / adjustment * adjustment, where
 * length is what the container restores to (as cdc_store_iterate_device
 * reports it).  Target-kind containers are counted too: the reference's
 * unwrap_chunk would panic on one, and a CDC fixture has none.  The non-empty
 * bins go to d_sizes / d_counts (DEVICE, cap entries) in ascending size order.
 * Returns the bin count; a return > cap means nothing was written.
 * CDC_EINVAL for adjustment == 0; CDC_ENOMEM if the bins (max length /
 * adjustment + 1 counters) cannot be allocated. */
int64_t cdc_store_size_distribution_device(cdc_store_t *st, uint64_t adjustment, uint64_t *d_sizes,
                                           uint32_t *d_counts, size_t cap, void *hip_stream);

/* ---- Removal and collection ---------------------------------------------------------
 * Not in the reference, whose store only grows: delete a file and get its space
 * in the arena back.  cdc_files_remove forgets a file on the host;
 * cdc_files_collect (and cdc_store_retain_device for users of the bare store)
 * then keeps exactly the containers that are still referenced, slides them down
 * the arena in place and rebuilds the table.
 *
 * After a collect with reference counts refs (for a layer: how many spans of its
 * files name the container; for cdc_store_retain_device: how often its digest is
 * given):
 *   a container stays if and only if refs > 0; its digest, length and bytes are
 *     unchanged, so get, contains and every file read return what they did.  A
 *     dropped digest is absent (contains 0, get CDC_ENOTFOUND) and a later put of
 *     the same bytes reports it new and stores it again;
 *   the survivors keep their relative arena order: the arena afterwards is their
 *     padded lengths back to back from 0 and arena_used is that sum.  The layout
 *     depends on the calls alone.  Where a length-0 container lies is unspecified;
 *   the stats are those of a store that had only ever been handed the surviving
 *     references: unique_chunks / unique_bytes are the survivors', chunks_written
 *     = sum of refs, bytes_written = sum of refs * length.  For a layer whose
 *     files were all written through it: what they would be had only the
 *     remaining files been written;
 *   the store's epoch is bumped (every cached slot and offset is stale).  The
 *     collecting layer rewrites the slot and offset of every span of its files
 *     and stamps them with the new epoch; a file that was stale already (written
 *     before a cdc_store_clear) is no root and stays stale.  A SECOND LAYER ON THE
 *     SAME STORE IS NOT CONSULTED: its containers are dropped unless the
 *     collecting layer names them too, and all its files return CDC_ENOTFOUND
 *     afterwards -- never wrong bytes.  Handles of cdc_store_retain_device's
 *     callers: every layer on the store goes stale.
 * A collect with nothing to drop moves no byte; it still rebuilds the table,
 * bumps the epoch and restamps the files (the stats may change: a removed file
 * whose chunks all live on in other files lowers chunks_written).
 *
 * A refused call changes nothing -- stats, epoch, every read, the arena bytes
 * below arena_used.  All refusals and every allocation come before the first
 * write to the table, the arena or a span table:
 *   CDC_EINVAL    a NULL layer, store or name, n > 0 with NULL digests;
 *   CDC_ENOTFOUND cdc_store_retain_device: a digest that is not stored;
 *   CDC_ENOMEM    a scratch allocation failed (the bounce buffer, the second set
 *                 of table arrays: 56 bytes per slot, about 150 bytes per
 *                 survivor);
 *   CDC_ENOTSUP   the store holds target-kind containers (it was scrubbed):
 *                 collecting key runs is not implemented.
 * Collecting a store that is another store's TARGET is allowed; the epoch bump
 * is what the base already treats as "target cleared".
 * A CDC_EDEVICE (a HIP error) once the move has begun leaves the store fit only
 * for cdc_store_clear or cdc_store_destroy.
 *
 * The move is in place: a group of survivors goes straight to its new offsets
 * when the whole group fits into the gap below it, and through a bounce buffer
 * otherwise.  The buffer is min(256 MiB, bytes to move), never below the longest
 * surviving container; CHUNKFS_AMD_GC_BOUNCE=bytes overrides the 256 MiB. */
typedef struct cdc_collect_stats {
    uint64_t containers_before;
    uint64_t containers_after;
    uint64_t arena_used_before;
    uint64_t arena_used_after;
    uint64_t bytes_moved;    /* padded bytes of the survivors that changed place */
    uint64_t groups_direct;  /* move groups copied arena -> arena */
    uint64_t groups_bounced; /* move groups that went through the bounce buffer */
    double seconds;          /* wall time of the call */
} cdc_collect_stats_t;

/* Drops the file `name` and returns its span table to the layer's pool.  Host
 * only: no device work, the store is not touched (cdc_files_collect reclaims
 * the space).  CDC_ENOTFOUND for an unknown name.  Handles to the file stay
 * allocated and every later call through them returns CDC_ENOTFOUND until a
 * file of that name is created again -- a new, empty file. */
int cdc_files_remove(cdc_files_t *fs, const char *name);

/* Keeps exactly the containers that some file of this layer references (see
 * above).  out is nullable. */
int cdc_files_collect(cdc_files_t *fs, cdc_collect_stats_t *out, void *hip_stream);

/* The same for users of the bare store: keeps exactly the containers whose
 * digest is among d_digests[0..n) (DEVICE, 32 bytes each; duplicates allowed,
 * each one counts as a reference; n = 0 keeps none).  Returns the number kept. */
int64_t cdc_store_retain_device(cdc_store_t *st, const uint8_t *d_digests, size_t n, void *hip_stream);

/* ---- Editing a file in place --------------------------------------------------------
 * Not in the reference, whose files only grow: replace the bytes [offset, offset +
 * remove_len) of a file with insert_len bytes from DEVICE memory (any alignment),
 * re-chunking only until the new cuts fall back onto the old ones.  One call covers
 * overwrite (remove_len == insert_len), insert (remove_len == 0), delete
 * (insert_len == 0), truncate (remove_len == size - offset, insert_len == 0) and
 * the append that re-chunks the old tail (offset == size).
 *
 * The rule.  Old spans have offsets off[0..n]; delta = insert_len - remove_len; C'
 * is the old content with the range replaced.
 *   1. i0 is the last span with off[i0] + 8 <= offset, or 0 if there is none (among
 *      equal offsets the last).  The 8 bytes cover AE, whose cut after byte i reads
 *      the bytes i .. i+3; every other rule reads nothing at or past its cut.
 *   2. T = chunk_data(C'[off[i0] ..]) with `chunker`, the whole tail as one buffer:
 *      cuts e_1 < e_2 < ... in the new file's coordinates.
 *   3. Resync: the smallest e_k >= offset + insert_len for which e_k - delta is an
 *      old boundary off[j]; the smallest such j.  The end of the file always is one.
 *   4. The new table: old spans [0, i0), the chunks of T up to e_k, old spans
 *      [j, n) with every offset moved by delta -- digests, slots and arena
 *      locations as they were.  An edit that leaves nothing after off[i0]
 *      (truncate to 0) inserts no span.
 * The engine does not chunk the whole tail: it chunks windows C'[off[i0], end_w)
 * and trusts a chunk of a window only if start + max + 8 <= end_w or the window
 * ends at the end of the file (max: the chunker's largest chunk, the chunk size
 * for FSChunker).  Round r = 1, 2, ... ends at min(size_after, offset + insert_len
 * + 4^r * max + 8); every round starts again from off[i0].  So a file written in
 * one call with chunker X and spliced with X has, span for span, the offsets and
 * digests of a file holding C' written in one call with X.
 *
 * The chunks up to e_k are hashed and put into the store; chunks of rounds that
 * did not resync are neither hashed nor stored.  The containers of the replaced
 * spans stay in the store until cdc_files_collect.  Other handles keep their
 * cursors as numbers.  The host waits for the device a fixed number of times per
 * round (the span search, the window read, the chunking, the resync) plus the
 * hash's, the put's and the final one -- never a number that grows with the file --
 * and an edit that resyncs in round 1 costs the window plus one pass over the
 * table (52 bytes per span; nothing but the replaced entries when the span count
 * and the size stay the same).
 *
 * Refusals, all before any device work, each leaving the file exactly as it was:
 *   CDC_EINVAL    a NULL handle, a NULL chunker, NULL data with insert_len > 0,
 *                 offset > size or offset + remove_len > size (no holes, no clipping);
 *   CDC_EPERM     a read-only handle;
 *   CDC_ENOTFOUND a removed file, or one whose spans predate a store clear;
 *   CDC_ENOTSUP   the store holds target-kind containers (it was scrubbed).
 * remove_len == 0 && insert_len == 0 returns 0 and touches nothing.  A put refused
 * with CDC_ENOMEM leaves the file and its table as they were: the put comes before
 * any write to the table.  Stream and epoch conventions are cdc_file_write_device's. */
typedef struct {
    uint64_t first_span;      /* i0: first span replaced */
    uint64_t spans_removed;   /* j - i0 */
    uint64_t spans_inserted;
    uint64_t resync_offset;   /* e_k, in the new file's coordinates (== new size if the cuts met only at the end) */
    uint64_t size_before, size_after;
    uint64_t bytes_new;       /* bytes the put stored for first-seen chunks */
    uint64_t window_bytes;    /* bytes handed to the chunker, all rounds together */
    uint32_t rounds;          /* chunking rounds (1 = the first window sufficed) */
    uint32_t pad;
} cdc_splice_stats_t;

/* Returns spans_inserted, or a negative CDC_E* code.  out is nullable. */
int64_t cdc_file_splice_device(cdc_fh_t *fh, cdc_handle_t *chunker, uint64_t offset, uint64_t remove_len,
                               const uint8_t *d_data, size_t insert_len, cdc_splice_stats_t *out,
                               void *hip_stream);

/* ---- Snapshots and diffs ------------------------------------------------------------
 * Not in the reference.  A snapshot is a copy of a span table -- 52 bytes per span
 * and no data byte -- and a diff rarely needs the data: two spans that name the
 * same store slot at the same file offset hold equal bytes by construction.
 * Together with splice, remove and collect: snapshot, edit in place, ask what
 * changed, drop the old version, collect.
 *
 * cdc_files_clone makes the file `dst` with a deep copy of `src`'s span table:
 * the same offsets, digests, slots and arena locations, the same size and epoch.
 * The table comes from the layer's pool in the smallest class that holds the
 * spans (not src's capacity); the copy is device-to-device on the call's stream,
 * with one host wait.  No put runs, no arena byte moves and the store's
 * statistics are unchanged; cdc_files_collect counts the clone's references like
 * any file's, so shared containers live as long as one version names them.  The
 * two files share nothing afterwards: an edit of either never shows through the
 * other.  A file without spans clones to a file without spans.  Works on a
 * scrubbed store (reads there go through the table's slots, which the clone
 * owns a copy of).  Returns the span count.  Refusals, each before any device
 * work and changing nothing:
 *   CDC_EINVAL    a NULL argument;
 *   CDC_ENOTFOUND an unknown src, or one whose spans predate a store clear;
 *   CDC_EEXIST    dst exists already (dst == src included);
 *   CDC_ENOMEM    the table could not be allocated.
 *
 * cdc_files_diff_device.  Let common = min(size_a, size_b) and D the positions x
 * in [0, max(size_a, size_b)) with x >= common or A[x] != B[x].  The answer is D
 * as its maximal runs {offset, length}: ascending, no two runs touch, no run is
 * empty -- canonical.  Returns the number of runs; d_ranges (DEVICE, cap entries)
 * is written only when that number is <= cap, otherwise nothing is written and
 * stats is still filled (cdc_file_distribution_device's convention).
 *   Pieces.  The distinct span boundaries of both tables inside (0, common) cut
 * [0, common) into pieces, each a non-empty interval inside one span of A and one
 * span of B.  Spans of length 0 add no piece.
 *   The sharing rule.  A piece is shared when its two spans have the same slot and
 * the same start offset, which is to say the two sides are one arena address.  A
 * shared piece is equal without being read.  Every other piece is compared byte
 * for byte -- also one whose spans have the same slot at different offsets.
 * Every compared byte of either file is read once; bytes_shared + bytes_compared
 * == common.
 *   CDC_DIFF_TABLES_ONLY.  No arena byte is read: every piece that is not shared
 * counts as differing, and the answer is the maximal runs of those pieces plus
 * the tail -- a superset of the exact answer for the price of the table pass, the
 * changed-chunks list of a backup.  bytes_compared == 0.
 * Read-only handles are fine; a and b on the same file give 0 runs with nothing
 * read; cursors are not touched.  The host waits for the device once.  Refusals,
 * each before any device work, leaving stats and d_ranges untouched:
 *   CDC_EINVAL    unknown flag bits, a NULL handle, cap > 0 with NULL d_ranges,
 *                 handles of two different layers;
 *   CDC_ENOTFOUND a removed file, or one whose spans predate a store clear;
 *   CDC_ENOTSUP   the store holds target-kind containers (it was scrubbed).
 * Stream convention: cdc_file_write_device's. */
typedef struct cdc_diff_stats {
    uint64_t ranges;          /* runs of the whole answer, also when it exceeds cap */
    uint64_t bytes_differing; /* sum of their lengths */
    uint64_t bytes_compared;  /* bytes of each file whose data was read */
    uint64_t bytes_shared;    /* bytes proved equal from the tables alone */
    uint64_t pieces;          /* pieces of [0, common); 0 when common == 0 */
    uint64_t size_a, size_b;
    double seconds;           /* wall time of the call */
} cdc_diff_stats_t;

#define CDC_DIFF_TABLES_ONLY 1u

/* Returns the span count of the new file, or a negative CDC_E* code. */
int64_t cdc_files_clone(cdc_files_t *fs, const char *src, const char *dst, void *hip_stream);

/* Returns the number of runs, or a negative CDC_E* code.  stats is nullable. */
int64_t cdc_files_diff_device(cdc_fh_t *a, cdc_fh_t *b, uint32_t flags, cdc_chunk_t *d_ranges, size_t cap,
                              cdc_diff_stats_t *stats, void *hip_stream);

/* ---- Content-aligned delta ----------------------------------------------------------
 * Not in the reference.  cdc_files_diff_device compares position by position, so
 * one inserted byte makes every later byte differ.  cdc_files_delta_device aligns
 * by content instead and returns an edit script that builds file B (new) out of
 * file A (old): an ordered list of ops that tile [0, size_b) exactly.
 *   COPY    {b_off, len, a_off}              B[b_off, b_off + len) == A[a_off, a_off + len);
 *   LITERAL {b_off, len, CDC_DELTA_LITERAL}  the bytes come from B.
 * COPY sources may overlap each other and appear in any order in A.  The store is
 * content-defined, so after an insert or delete the chunker falls back onto the
 * old cuts within a few spans and every later span of B names the same store slot
 * as a span of A at a shifted offset: the tables give the alignment, a few
 * kilobytes around the edit give the exact edges.
 *   The rule is deterministic.  Spans of length 0 hold no byte and take no part.
 *   1. Anchors (tables only).  B's span j matches when some span of A has the same
 * slot.  Among A's spans with that slot the one taken is the span i that minimises
 * |off_a[i] - off_b[j]|; on a tie the smaller off_a[i] wins.  Its diagonal is
 * off_a[i] - off_b[j].  An unchanged region is a diagonal-0 copy, and a run of one
 * repeated chunk stays on one diagonal.
 *   2. Runs.  Consecutive matched spans of B with the same diagonal form one COPY;
 * consecutive unmatched spans form one LITERAL region [l, r).  With
 * CDC_DELTA_TABLES_ONLY this is the answer, and no arena byte is read.
 *   3. Edges (exact mode).  Each region is set against its neighbours' diagonals:
 * dL is the left COPY's diagonal, or 0 when the region begins the file; dR is the
 * right COPY's diagonal, or size_a - size_b when the region ends the file -- so
 * two files that share no slot still get their common prefix and suffix.  e is the
 * largest value <= r - l with B[l + k] == A[l + dL + k] for all k < e; it stops
 * where the A index leaves [0, size_a).  f is the largest value <= (r - l) - e with
 * B[r - 1 - k] == A[r - 1 - k + dR] for all k < f, under the same bound: forward
 * takes precedence.  The region becomes COPY e, LITERAL r - l - e - f, COPY f.
 *   4. Canonical form.  Ops of length 0 are dropped; adjacent COPYs on one diagonal
 * are merged (a region that vanishes joins its neighbours); after that no two
 * LITERALs are adjacent.
 * Returns the number of ops; d_ops (DEVICE, cap entries) is written only when that
 * number is <= cap, otherwise nothing is written and stats is still filled
 * (cdc_files_diff_device's convention).  bytes_copy + bytes_literal == size_b.
 * bytes_literal_tables is the LITERAL bytes after step 2: it bounds what step 3
 * reads.  Read-only handles are fine; cursors are not touched; a and b on the same
 * file give one COPY with a_off == 0, or no op when the file is empty.  With
 * size_a == 0 the answer is one LITERAL, with size_b == 0 no op, and neither
 * runs a device pass.  The host waits for the device once.  Refusals, each before
 * any device work, leaving stats and d_ops untouched:
 *   CDC_EINVAL    unknown flag bits, a NULL handle, cap > 0 with NULL d_ops,
 *                 handles of two different layers;
 *   CDC_ENOTFOUND a removed file, or one whose spans predate a store clear;
 *   CDC_ENOTSUP   the store holds target-kind containers (it was scrubbed).
 * Stream convention: cdc_file_write_device's. */
typedef struct cdc_delta_op {
    uint64_t b_off; /* where the op's bytes lie in B */
    uint64_t len;
    uint64_t a_off; /* COPY: where they lie in A; LITERAL: CDC_DELTA_LITERAL */
} cdc_delta_op_t;

typedef struct cdc_delta_stats {
    uint64_t ops;                  /* ops of the whole script, also when it exceeds cap */
    uint64_t bytes_copy;           /* bytes of the COPY ops */
    uint64_t bytes_literal;        /* bytes of the LITERAL ops */
    uint64_t bytes_literal_tables; /* LITERAL bytes after step 2 */
    uint64_t spans_matched;        /* spans of B with bytes whose slot A names too */
    uint64_t regions;              /* LITERAL regions after step 2 */
    uint64_t size_a, size_b;
    double seconds;                /* wall time of the call */
} cdc_delta_stats_t;

#define CDC_DELTA_LITERAL (~0ull) /* a_off of a LITERAL op */
#define CDC_DELTA_TABLES_ONLY 1u

/* Returns the number of ops, or a negative CDC_E* code.  stats is nullable. */
int64_t cdc_files_delta_device(cdc_fh_t *a, cdc_fh_t *b, uint32_t flags, cdc_delta_op_t *d_ops, size_t cap,
                               cdc_delta_stats_t *stats, void *hip_stream);

/* ---- Packs: send and receive ----------------------------------------------------------
 * Not in the reference.  A pack is one file of the layer as a self-describing,
 * deduplicated, deterministic byte image, built and consumed on the device: what
 * a store sends to another store -- on the same GPU, on another GPU, or through a
 * disk file to a later process -- so that only the chunks the other side lacks
 * move, and nothing is chunked or (with CDC_UNPACK_TRUST) hashed again.
 *
 * The format, version 1, little-endian, every section at a 16-byte multiple:
 *   header, 64 bytes:
 *     u64 magic          the bytes "CDCPACK1"
 *     u32 version = 1    u32 flags = 0 (reserved, must be 0)
 *     u64 file_size      u64 n_spans
 *     u64 n_chunks       containers carried in the pack
 *     u64 external_spans spans whose chunk the pack does not carry
 *     u64 data_bytes     size of the data section
 *     u64 total_bytes    the whole pack
 *   span_digest  [n_spans][32]  the file's digests in file order (cdc_file_hashes_device)
 *   span_length  [n_spans] u64
 *   span_chunk   [n_spans] u64  index k of the carried chunk holding this span's bytes, ~0 = external
 *   chunk_span   [n_chunks] u64 span index of carried chunk k's first occurrence; strictly increasing
 *   chunk_off    [n_chunks + 1] u64  exclusive scan of round_up(length, 16), relative to the data section
 *   data         [data_bytes]   carried chunks back to back at 16-byte multiples
 * Every padding byte, between sections and after each chunk, is zero: two packs of
 * the same file with the same exclusions are byte-identical.  Carried chunks are
 * the file's distinct slots that are not excluded, in order of first occurrence in
 * the file -- the order in which a put lays them out.  Length-0 spans are legal.
 * A file without spans packs to its header alone, 64 bytes, with no section.
 *
 * cdc_file_pack_device.  A slot is excluded when some span of `since` names it
 * (nullable: a handle of the same layer, typically a clone taken before edits),
 * or some span i of the file that names it has d_have[i] != 0 (nullable: DEVICE
 * u8[spans], the receiver's cdc_store_contains_device answer to this file's
 * cdc_file_hashes_device).  since == fh is legal and carries nothing.  Returns
 * total_bytes (snprintf convention: a return > cap means NOTHING was written;
 * cap = 0 sizes a pack without copying a data byte; stats is filled either way).
 * d_pack: DEVICE, 16-byte aligned.  Cursors are untouched, read-only handles are
 * fine.  The host waits for the device twice: for the sizes, and at the end.
 * Refusals, each before any device work and changing nothing:
 *   CDC_EINVAL    a misaligned d_pack, a NULL handle, cap > 0 with NULL d_pack,
 *                 `since` of another layer;
 *   CDC_ENOTFOUND a removed file, or one whose spans predate a store clear, on
 *                 either handle;
 *   CDC_ENOTSUP   the store holds target-kind containers (it was scrubbed).
 *
 * cdc_files_unpack_device creates the file `name` from the len bytes at d_pack
 * (DEVICE, 16-byte aligned) and returns its span count.  `hasher` is any chunker
 * handle on the store's device (its engine owns the SHA-256 workspaces); NULL only
 * with CDC_UNPACK_TRUST.  The pack is untrusted input: no kernel reads outside
 * [d_pack, d_pack + len) or indexes outside a section, whatever the bytes say.
 * The checks, in this order, every one before the first write to the store or the
 * layer -- a refused call changes nothing, stats included:
 *   1. arguments: CDC_EINVAL for unknown flag bits, a misaligned pack, len < 64,
 *      a NULL argument, a hasher on another device; CDC_EEXIST if `name` exists;
 *      CDC_ENOTSUP on a scrubbed store;
 *   2. structure, CDC_EINVAL with the check and the first offending index in
 *      cdc_last_error(): on the host magic, version, flags, every section size
 *      recomputed from n_spans / n_chunks without overflow, total_bytes <= len;
 *      then one kernel: chunk_span strictly increasing and < n_spans; span_chunk
 *      ~0 or < n_chunks; span_chunk[chunk_span[k]] == k; every carried span equal
 *      in digest and length to the first span of its chunk; chunk_off[0] == 0 with
 *      steps of round_up(length, 16); chunk_off[n_chunks] == data_bytes; the
 *      lengths sum to file_size; external_spans counts the ~0 entries;
 *   3. externals: every external span's digest is in the store, else
 *      CDC_ENOTFOUND naming the first missing span (and CDC_EINVAL if the store
 *      holds it with another length than the pack states);
 *   4. integrity, unless CDC_UNPACK_TRUST: one cdc_sha256_batch_device over the
 *      carried chunks, compared with their digests; a mismatch is CDC_EINVAL naming
 *      the chunk.  With CDC_UNPACK_TRUST nothing is hashed: a corrupted data byte
 *      is stored as it is, under the digest the pack states;
 *   5. the put of the carried chunks, with its own refusals (CDC_ENOMEM "as if
 *      every chunk were new").  First insert wins: a carried chunk the store holds
 *      already adds nothing.
 * Then every span gets its slot, the table is built as an append builds it, and
 * the file is registered.  The store's chunks_written and bytes_written count
 * every span of the file, as a write of the same content would.  Unpacking a full
 * pack into an empty store gives exactly the store and the file that one
 * cdc_file_write_device of the content with the sender's chunker gives: digests,
 * span offsets, bytes and every field of cdc_store_stats, arena_used included.
 * Stream convention: cdc_file_write_device's. */
typedef struct cdc_pack_stats {
    uint64_t spans;          /* spans of the file */
    uint64_t chunks;         /* carried chunks */
    uint64_t external_spans; /* spans whose chunk the pack does not carry */
    uint64_t chunk_bytes;    /* unpadded sum of the carried lengths */
    uint64_t pack_bytes;     /* the whole pack */
    uint64_t file_size;      /* bytes of the file */
    uint64_t chunks_new;     /* unpack: carried chunks the receiver did not hold; pack: 0 */
    double seconds;          /* wall time of the call */
} cdc_pack_stats_t;

#define CDC_UNPACK_TRUST 1u /* skip the SHA-256 check of the carried chunks */

/* Returns total_bytes, or a negative CDC_E* code.  since, d_have and stats are nullable. */
int64_t cdc_file_pack_device(cdc_fh_t *fh, cdc_fh_t *since, const uint8_t *d_have, uint8_t *d_pack, size_t cap,
                             cdc_pack_stats_t *stats, void *hip_stream);

/* Returns the span count of the new file, or a negative CDC_E* code.  stats is nullable. */
int64_t cdc_files_unpack_device(cdc_files_t *fs, const char *name, const uint8_t *d_pack, size_t len,
                                cdc_handle_t *hasher, uint32_t flags, cdc_pack_stats_t *stats, void *hip_stream);

/* ---- Synthetic data -----------------------------------------
 * Fill a DEVICE buffer with the splitmix64 stream: little-endian u64 words,
 * word i = mix64(seed + (i+1) * 0x9E3779B97F4A7C15). */
int cdc_fill_splitmix64_device(uint8_t *d_buf, size_t len, uint64_t seed,
                               void *hip_stream);

/* Engine build info, e.g. "chunkfs_amd 0.5 gfx950 abi 3". */
const char *cdc_version(void);

/* CHUNKFS_AMD_ABI_VERSION of the loaded library (compare with the header's). */
uint32_t cdc_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CHUNKFS_AMD_H */
