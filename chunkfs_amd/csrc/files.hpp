// files.hpp -- device file layer kernels (files.hip) and their host object
// (files_host.cpp): per-file span tables in HBM over the chunk store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "read_plan.hpp"
#include "store.hpp"

namespace cdc {

// One file's span table, structure of arrays in HBM.  Span i covers the bytes
// [off[i], off[i + 1]) of the file; off[0] = 0 and off[n] = the file's size.
struct SpanTable {
    uint64_t *off;     // [cap + 1]
    uint8_t *digest;   // [cap * 32]
    uint64_t *loc;     // [cap] arena offset of the span's bytes (the store's loc[slot])
    uint32_t *slot;    // [cap] the span's table slot (the distribution counts per slot)
};

// One read request, built on the host (kind: ReadKind, read_plan.hpp).
struct ReadReq {
    const uint64_t *off;
    const uint64_t *loc;
    uint64_t n;      // spans of the file
    uint64_t a;      // segment: the cursor; range: the offset
    uint64_t b;      // segment: the segment size; range: the length
    uint64_t dst;    // device address of the request's first byte
    uint64_t cap;    // bytes the destination holds
    uint64_t spans;  // complete only: device address of cdc_chunk_t[n], or 0
    uint32_t kind;
    uint32_t pad;
};

// What the planner leaves per request (device scratch; `bytes`, `first` and
// `count` also go to the host result block).
struct ReadPlan {
    uint64_t lo, hi;  // byte range of the file
    uint64_t first;   // first span
};
struct ReadResult {
    uint64_t bytes;  // what the request yields (also when it exceeds cap: nothing is copied then)
    uint64_t first;
    uint64_t count;  // spans the request touches
};

// Append n spans to a table holding n0 spans and size0 bytes, after a put of the
// same n chunks: slot_of is the put's slot list.  val: n u64 scratch, block_sums:
// store_scan_blocks(n) + 1.  *h_total (pinned host) = bytes appended.  d_stat
// (device, preset to {~0, 0}): [0] = min(length - 1) over the spans of length >
// 0, [1] += spans of length 0.
hipError_t launch_files_append(const SpanTable &t, uint64_t n0, uint64_t size0, const uint32_t *slot_of,
                               const uint64_t *tbl_length, const uint64_t *tbl_loc, const uint8_t *d_digests,
                               uint64_t n, uint64_t *val, uint64_t *block_sums, unsigned long long *d_stat,
                               unsigned long long *h_total, hipStream_t s);

// The segmented append of cdc_files_write_batch_device: the m = first[nfiles]
// spans of one batch put go to nfiles tables in one pass.  File f owns spans
// [first[f], first[f + 1]) (files without spans make runs of equal entries) and
// receives them from entry n0 on, its offsets continuing from size0; its table
// must have room for n0 + first[f + 1] - first[f] spans.
struct AppendDst {
    SpanTable t;
    uint64_t n0;
    uint64_t size0;
};
// Per file, preset to {0, ~0, 0}: bytes appended, min(length - 1) over the spans
// of length > 0, spans of length 0 (launch_files_append's *h_total and d_stat).
struct AppendStat {
    unsigned long long bytes, least, zeros;
};
// d_dst / d_first / d_stat: device arrays of nfiles, nfiles + 1, nfiles entries;
// slot_of .. block_sums as launch_files_append, over the m spans.  One scan over
// all m lengths, no host wait; the caller copies d_stat back.
hipError_t launch_files_append_batch(const AppendDst *d_dst, const uint64_t *d_first, uint64_t nfiles, uint64_t m,
                                     const uint32_t *slot_of, const uint64_t *tbl_length, const uint64_t *tbl_loc,
                                     const uint8_t *d_digests, uint64_t *val, uint64_t *block_sums,
                                     AppendStat *d_stat, hipStream_t s);

// The range planner and the copy: nreq requests -> span ranges -> pieces ->
// tiles -> copy_kernel, with no host wait in between.  max_pieces / max_tiles
// are host-side bounds (they size grids and scratch; a bound below the true
// count would drop pieces); the exact counts stay on the device.  plan: nreq;
// cnt: nreq u64; rblock: store_scan_blocks(nreq) + 1; pieces / tstart:
// max_pieces; block_sums: store_scan_blocks(max_pieces) + 1; h_res: nreq results
// in pinned host memory.  With d_diff (device u64, preset to ~0) the last step is
// the store's compare instead of its copy (cdc_file_verify_device): the
// requests' destinations are read, not written, and *d_diff receives the
// smallest destination address - cmp_base at which a byte differs.
hipError_t launch_files_read(const ReadReq *d_req, uint64_t nreq, uint64_t arena, ReadPlan *plan, uint64_t *cnt,
                             uint64_t *rblock, StorePiece *pieces, uint64_t *tstart, uint64_t *block_sums,
                             uint64_t max_pieces, uint64_t max_tiles, ReadResult *h_res, hipStream_t s,
                             uint64_t cmp_base = 0, unsigned long long *d_diff = nullptr);

// ---- reads in the scrubbed state ------------------------------------------------
// Once the store holds target-kind containers a span's bytes are found through
// its slot's current container (ScrubView, store.hpp): the same chain with one
// more level, span -> pieces.  One record per span a request touches.
struct SpanRec {
    uint64_t s0;        // the span's first byte in the file
    uint64_t from, to;  // the part of it the request takes
    uint64_t dst0;      // destination address of file byte 0: a file byte x goes to dst0 + x
    uint64_t key0;      // first key taken of a target-kind span; ~0 for a chunk-kind span
    uint32_t slot;
    uint32_t pad;
};

// Steps 1-3: requests -> span ranges (as launch_files_read) -> one SpanRec and
// piece count per span: a chunk-kind span is one piece, a target-kind span one
// piece per key, and a range read trims its first and last span by binary
// search over the per-key offsets inside the container.  d_rslot[r] = device
// address of request r's slot array.  max_spans is the host-side bound
// launch_files_read calls max_pieces; recs / pcnt: max_spans; pblock:
// store_scan_blocks(max_spans) + 1.  h_tot (pinned host): [0] = pieces in all,
// [1] = target-kind spans touched -- the host reads both before the copy, so
// the piece scratch is sized exactly and a cleared target is refused before a
// byte is written.
hipError_t launch_files_plan_x(const ReadReq *d_req, const uint64_t *d_rslot, uint64_t nreq, const ScrubView &v,
                               ReadPlan *plan, uint64_t *cnt, uint64_t *rblock, SpanRec *recs, uint64_t *pcnt,
                               uint64_t *pblock, uint64_t max_spans, ReadResult *h_res,
                               unsigned long long *d_touch, unsigned long long *h_tot, hipStream_t s);

// Steps 4-6 after the host has read h_tot: the n_pieces pieces, the tile scan
// and the store's copy.  pcnt is the scan launch_files_plan_x left; pieces /
// tstart: n_pieces; block_sums: store_scan_blocks(n_pieces) + 1.  d_diff /
// cmp_base: the compare instead of the copy, as in launch_files_read.
hipError_t launch_files_copy_x(const SpanRec *recs, const uint64_t *pcnt, uint64_t max_spans, const ScrubView &v,
                               const uint64_t *loc, uint64_t arena, StorePiece *pieces, uint64_t *tstart,
                               uint64_t *block_sums, uint64_t n_pieces, uint64_t max_tiles, hipStream_t s,
                               uint64_t cmp_base = 0, unsigned long long *d_diff = nullptr);

// chunk_count_distribution over spans [0, m), m = n - 1: per distinct slot, in
// order of first occurrence, {digest, count, off[i + 1] - off[i] of the first
// occurrence}.  cnt / firstpos: table-sized scratch (only the slots the file
// uses are initialised); val: m; block_sums: store_scan_blocks(m) + 1.  Nothing
// is written when the distinct count exceeds cap; *h_distinct (pinned) gets it.
hipError_t launch_files_distribution(const SpanTable &t, uint64_t m, uint32_t *cnt, uint64_t *firstpos,
                                     uint64_t *val, uint64_t *block_sums, uint8_t *d_digests, uint32_t *d_counts,
                                     uint64_t *d_lengths, uint64_t cap, unsigned long long *h_distinct,
                                     hipStream_t s);

// ---- collect (cdc_files_collect) ----------------------------------------------------
// One file of the layer: the slot and arena-offset arrays of its span table.
struct CollectSeg {
    uint32_t *slot;
    uint64_t *loc;
};
// The reference pass: all m = first[nfiles] spans of the layer's files in one
// launch, file f owning spans [first[f], first[f + 1]) (d_seg: nfiles entries,
// d_first: nfiles + 1, both DEVICE).  refs[slot] += 1 per span (refs: `slots`
// u64, zeroed by the caller), combined within the wave before the atomics.
hipError_t launch_files_refs(const CollectSeg *d_seg, const uint64_t *d_first, uint64_t nfiles, uint64_t m,
                             uint64_t slots, unsigned long long *refs, hipStream_t s);
// After store_retain: slot[i] = map[slot[i]], loc[i] = new_loc[slot[i]] for every span.
hipError_t launch_files_remap(const CollectSeg *d_seg, const uint64_t *d_first, uint64_t nfiles, uint64_t m,
                              uint64_t slots, const uint32_t *map, const uint64_t *new_loc, hipStream_t s);

// ---- splice (cdc_file_splice_device; the arithmetic: splice_plan.hpp) -------------
// Step 1: h_out (pinned) = {i0, off[i0]} of a table holding n > 0 spans.
hipError_t launch_splice_start(const uint64_t *off, uint64_t n, uint64_t offset, unsigned long long *h_out,
                               hipStream_t s);

// What one round's resync needs besides the table: the window [w0, end_w) of the
// new file that was chunked, and the edit.
struct SpliceRound {
    uint64_t w0, end_w;
    uint64_t size_after;
    uint64_t offset, remove_len, insert_len;
    uint64_t max_chunk;
};
// Step 3 over the m > 0 chunks of a window (offsets relative to w0): the smallest
// trusted k whose cut e_k >= offset + insert_len lies on an old boundary.  d_best:
// one device word.  h_out (pinned) = {k, j, e_k}, k = ~0 when no chunk qualifies.
hipError_t launch_splice_resync(const cdc_chunk_pod *chunks, uint64_t m, const SpliceRound &r, const uint64_t *off,
                                uint64_t n, unsigned long long *d_best, unsigned long long *h_out, hipStream_t s);

// Step 4 after the put of the m accepted chunks (slot_of .. d_stat, h_total as
// launch_files_append): dst = old spans [0, i0), the m chunks from offset w0 on,
// old spans [j, n) with off + (ins - rem); dst.off[n_new] closes the table, n_new
// = i0 + m + n - j.  dst must not overlap old -- unless m == j - i0 and ins ==
// rem, when dst may BE old: then only the entries [i0, i0 + m) are written.
// size_old = old.off[n]: a file without spans has no table to read it from.
hipError_t launch_splice_build(const SpanTable &old, uint64_t n, uint64_t size_old, const SpanTable &dst,
                               uint64_t i0, uint64_t j, uint64_t w0, uint64_t rem, uint64_t ins, const uint32_t *slot_of,
                               const uint64_t *tbl_length, const uint64_t *tbl_loc, const uint8_t *d_digests,
                               uint64_t m, uint64_t *val, uint64_t *block_sums, unsigned long long *d_stat,
                               unsigned long long *h_total, hipStream_t s);

// ---- diff (cdc_files_diff_device; the arithmetic: diff_plan.hpp) -------------------
// One file of the two: its table and size.  Both have spans (common > 0).
struct DiffSide {
    const uint64_t *off;
    const uint64_t *loc;
    const uint32_t *slot;
    uint64_t n;
    uint64_t size;
};
// Device scratch, sized from host-side bounds: nc = na + nb + 2 candidates,
// max_pieces = na + nb, max_tiles = common / kStoreTile + 2 * max_pieces (0 for
// CDC_DIFF_TABLES_ONLY: tcount and mask are not touched then).
struct DiffScratch {
    uint64_t *cand;    // [nc] do the candidates open a piece; scanned
    uint64_t *pstart;  // [max_pieces] the pieces in file order: first byte
    uint32_t *pia;     // [max_pieces] A's span
    uint32_t *pib;     // [max_pieces] B's span
    uint64_t *pflag;   // [max_pieces] exact: the piece is compared; tables only: it begins a run; scanned
    StorePiece *cp;    // [max_pieces] the compared pieces: {A's address, B's address, length}
    uint64_t *tstart;  // [max_pieces] their tile counts; scanned
    uint64_t *cx;      // [max_pieces] their first byte in the file
    uint32_t *cflag;   // [max_pieces] bit 0: the piece before it in the file is compared too; bit 1: it ends at
                       // `common` and the files differ in size
    uint64_t *tcount;  // [max_tiles] run starts per tile; scanned
    uint64_t *mask;    // [64 * max_tiles]
    uint64_t *bs_c, *bs_p, *bs_t, *bs_r;  // block sums of the four scans: store_scan_blocks(count) + 1 each
    // Their totals, the last entry of each: pieces, compared pieces (tables only: runs below `common`),
    // tiles, runs that begin below `common`.
    const uint64_t *n_pieces, *n_cmp, *n_tiles, *n_starts;
    unsigned long long *acc;  // [4]: bytes of the pieces not shared, differing bytes below `common`, ranges,
                              // whether the tail continues a run
    uint64_t max_pieces, max_tiles;
};
// The whole device path, no host wait inside.  h_out (pinned): [0] ranges, [1]
// bytes_differing, [2] bytes_compared, [3] bytes_shared, [4] pieces.  d_ranges
// receives the ranges when their number is <= cap, and is left alone otherwise.
hipError_t launch_files_diff(const DiffSide &a, const DiffSide &b, uint64_t arena, bool tables_only,
                             const DiffScratch &w, cdc_chunk_pod *d_ranges, uint64_t cap, unsigned long long *h_out,
                             hipStream_t s);

// ---- get_to_dedup_ratio (file_layer.rs:208-268) -----------------------------------
// Step 1: the unique list over spans [0, m), m = n - 1, from the distribution's
// first-occurrence flags and scan: uidx[j] = span index of the j-th distinct
// slot, ulen = the exclusive scan of their lengths over m entries (zero past
// the unique count; the total in ublock[store_scan_blocks(m)]).  cnt / firstpos
// / val / block_sums as launch_files_distribution; uidx / ulen: m; ublock:
// store_scan_blocks(m) + 1.  h_out (pinned): [0] = U, [1] = unique_length.
hipError_t launch_files_ratio_unique(const SpanTable &t, uint64_t m, uint32_t *cnt, uint64_t *firstpos, uint64_t *val,
                                     uint64_t *block_sums, uint64_t *uidx, uint64_t *ulen, uint64_t *ublock,
                                     unsigned long long *h_out, hipStream_t s);

// Step 2, once the host has R and total_size: h_out[0] = C = bytes of one cycle
// over the first R unique entries, h_out[1] = entries the take-while accepts of
// the last, partial cycle.
hipError_t launch_files_ratio_take(const uint64_t *pre, const uint64_t *ublock, uint64_t m, uint64_t R,
                                   uint64_t total_size, unsigned long long *h_out, hipStream_t s);

// Step 3: the n = K + (U - R) spans of the derived file into dst (room for n):
// span i < K is unique entry i mod R, span i >= K entry R + i - K; offsets are
// the scan of the gathered lengths; digest, slot and loc are the source's.
// sidx / val: n; block_sums: store_scan_blocks(n) + 1; d_stat as
// launch_files_append; *h_total (pinned) = the new file's size.
hipError_t launch_files_ratio_gather(const SpanTable &src, const SpanTable &dst, const uint64_t *uidx, uint64_t K,
                                     uint64_t R, uint64_t n, uint64_t *sidx, uint64_t *val, uint64_t *block_sums,
                                     unsigned long long *d_stat, unsigned long long *h_total, hipStream_t s);

}  // namespace cdc
