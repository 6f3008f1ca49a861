// store.hpp -- device chunk store kernels (store.hip) and their host object
// (store_host.cpp): the dedup index plus an HBM arena of first-seen chunks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index.hpp"

namespace cdc {

constexpr uint64_t kStoreAlign = 16;     // stored chunks start at 16-byte multiples
constexpr uint64_t kStoreTile = 4096;    // destination bytes one wave copies
constexpr uint64_t kScanBlockItems = 2048;  // items one block of the scan covers

// One variable-length copy: len bytes from src to dst (device addresses).
struct StorePiece {
    uint64_t src;
    uint64_t dst;
    uint64_t len;
};

// Blocks the scan needs for n items (size of its d_block_sums scratch).
inline uint64_t store_scan_blocks(uint64_t n) { return (n + kScanBlockItems - 1) / kScanBlockItems; }

// put, step 1: chunk i of stream j (first[j] <= i < first[j+1]; d_first has
// n_streams + 1 entries) must lie inside [0, lens[j]).  d_acc[0] += chunks out
// of bounds, d_acc[1] += sum of round_up(length, 16), d_acc[2] += sum of
// ceil(length / kStoreTile), d_acc[3] += times the sum in d_acc[1] passed 2^64
// (saturated inside a wave first).  pieces[i] = {source address, 0, length}
// for the chunks in bounds ({0, 0, 0} otherwise).
hipError_t launch_store_precheck(const void *d_chunks, uint64_t n, const uint64_t *d_streams,
                                 const uint64_t *d_lens, const uint64_t *d_first, uint64_t n_streams,
                                 StorePiece *pieces, unsigned long long *d_acc, hipStream_t s);

// put, step 3 (after launch_index_insert): arena offsets of the new chunks
// (exclusive scan of padded lengths over the new flags, from arena_used), the
// slot's loc entry, and the copy into the arena.  val / tstart: n u64 scratch
// each; block_sums: store_scan_blocks(n) + 1 u64.  max_tiles bounds the tile count
// (d_acc[2] of the precheck); *d_taken = arena bytes the new chunks take.
hipError_t launch_store_compact(uint8_t *arena, uint64_t arena_used, uint64_t *loc, const uint32_t *d_slot_of,
                                const uint8_t *d_new, StorePiece *pieces, uint64_t n, uint64_t *val,
                                uint64_t *tstart, uint64_t *block_sums, uint64_t max_tiles,
                                unsigned long long *d_taken, hipStream_t s);

// get / contains, step 1: one thread per digest.  Full 32-byte comparison,
// probing past tag matches of another digest.  pieces[i] = {arena address, 0,
// length} ({0, 0, 0} when absent); found (nullable) receives 1/0; d_res[0] +=
// digests absent.
hipError_t launch_store_lookup(const IndexTable &t, const uint64_t *loc, const uint8_t *arena,
                               const uint8_t *d_digests, uint64_t n, StorePiece *pieces, uint8_t *found,
                               unsigned long long *d_res, hipStream_t s);

// get, step 2: destinations d_out + exclusive scan of the lengths, tile counts
// and their scan.  d_res[1] = total bytes, d_res[2] = total tiles.
hipError_t launch_store_plan_get(StorePiece *pieces, uint64_t n, uint64_t d_out, uint64_t *val, uint64_t *tstart,
                                 uint64_t *block_sums, unsigned long long *d_res, hipStream_t s);

// get, step 3 (after the host has checked d_res): the copy, and the spans.
hipError_t launch_store_gather(const StorePiece *pieces, const uint64_t *tstart, uint64_t n, uint64_t tiles,
                               uint64_t d_out, void *d_spans, hipStream_t s);

// For the file layer (files.hip): the exclusive scan of v[0, n) in place
// (block_sums: store_scan_blocks(n) + 1 u64, the total left in block_sums[blocks]
// and in *total_out when given), and the copy over a caller-built piece list
// whose tile scan is tstart; the tile total is read on the device from
// *d_total, max_tiles (a host-side bound) only sizes the grid.
hipError_t launch_store_scan(uint64_t *v, uint64_t n, uint64_t *block_sums, unsigned long long *total_out,
                             hipStream_t s);
hipError_t launch_store_copy(const StorePiece *pieces, const uint64_t *tstart, uint64_t n, uint64_t max_tiles,
                             const uint64_t *d_total, hipStream_t s);

// The compare over the same kind of piece list (cdc_file_verify_device): piece
// {src, dst, len} says that the caller's bytes at dst should equal the arena's
// at src.  Nothing is written but *d_diff (device, preset to ~0): the smallest
// dst - base at which a byte differs.  Loads on the dst side stay inside the
// pieces; the src side follows the copy's over-read rule.
hipError_t launch_store_compare(const StorePiece *pieces, const uint64_t *tstart, uint64_t n, uint64_t max_tiles,
                                const uint64_t *d_total, uint64_t base, unsigned long long *d_diff, hipStream_t s);

// The difference mask over the same kind of piece list (cdc_files_diff_device):
// piece {src, dst, len} names the two sides, both read and neither written.
// Tile w of the tile scan owns mask[64 w, 64 w + 64): bit b stands for the byte
// at (dst & ~15) + k * kStoreTile + b of its piece's tile k, set where the sides
// differ, zero outside the piece.  mask: 64 words per tile of max_tiles.  Loads
// follow the compare's rule on either side.
hipError_t launch_store_diff_mask(const StorePiece *pieces, const uint64_t *tstart, uint64_t n, uint64_t max_tiles,
                                  const uint64_t *d_total, uint64_t *mask, hipStream_t s);

// Size distribution (CDCFixture::size_distribution, src/bench/mod.rs:218-232).
// Step 1: *d_max (preset to 0) = the longest container over the occupied slots.
hipError_t launch_store_dist_max(const IndexTable &t, unsigned long long *d_max, hipStream_t s);
// Step 2: bins[length / adjustment] += 1 per occupied slot (bins: n_bins u32,
// zeroed; aggregated within the wave before the atomics), val = the scanned
// non-empty flags, *d_total = non-empty bins.  val: n_bins; block_sums:
// store_scan_blocks(n_bins) + 1.
hipError_t launch_store_dist_bins(const IndexTable &t, uint64_t adjustment, uint32_t *bins, uint64_t n_bins,
                                  uint64_t *val, uint64_t *block_sums, unsigned long long *d_total, hipStream_t s);
// Step 3: the non-empty bins in ascending order: {bin * adjustment, count}.
hipError_t launch_store_dist_emit(const uint32_t *bins, uint64_t n_bins, const uint64_t *val, uint64_t adjustment,
                                  uint64_t *d_sizes, uint32_t *d_counts, hipStream_t s);

// ---- scrub stage ---------------------------------------------------------------
// The base store's view of its containers once a target store is attached
// (DataContainer, src/system/storage.rs:12-21): kind[slot] = 0 for a chunk, 1
// for a list of target keys; a target-kind slot owns the run [key_first,
// key_first + key_count) of the key arrays.  Keys are stored resolved: the
// target store's slot, and the byte offset of the key's value inside the
// container it restores.  t_* are the target store's arrays.
struct ScrubView {
    const uint8_t *kind;
    const uint64_t *key_first;
    const uint32_t *key_count;
    const uint32_t *key_slot;
    const uint64_t *key_off;
    const uint64_t *t_length;
    const uint64_t *t_loc;
    const uint8_t *t_digest;
    uint64_t t_arena;
};

// The writable side of the same arrays (the marking kernel).
struct ScrubState {
    uint8_t *kind;
    uint64_t *key_first;
    uint32_t *key_count;
    uint32_t *key_slot;
    uint64_t *key_off;
};

// scrub, step 1: val[s] = 1 for the occupied chunk-kind slots (`want_kind` 0)
// or for every occupied slot (`want_kind` < 0), scanned in place; *d_total =
// how many.  val: slots u64, block_sums: store_scan_blocks(slots) + 1.
hipError_t launch_scrub_flag(const IndexTable &t, const uint8_t *kind, int want_kind, uint64_t *val,
                             uint64_t *block_sums, unsigned long long *d_total, hipStream_t s);

// scrub, step 1b: the container list in slot order from the scanned flags:
// chunks[j] = {arena offset, length}, digests[j], slot_of[j]; *d_bytes += the
// lengths.
hipError_t launch_scrub_list(const IndexTable &t, const uint8_t *kind, const uint64_t *loc, const uint64_t *val,
                             void *d_chunks, uint8_t *d_digests, uint32_t *d_slot, unsigned long long *d_bytes,
                             hipStream_t s);

// RECHUNK planning: *d_sum += sum of round_up(length, 16) over n chunks.
hipError_t launch_scrub_padsum(const void *d_chunks, uint64_t n, unsigned long long *d_sum, hipStream_t s);

// scrub, step 4: containers [0, nc) of a group (slots c_slot) become
// target-kind; container j owns keys [first[j], first[j + 1]) of the group's n
// keys (d_first NULL: one key each, key j), written from key_base on.  Key i
// is the target slot t_slot[i] at offset d_sub[i].offset inside its container
// (d_sub NULL: 0).
hipError_t launch_scrub_mark(const ScrubState &w, const uint32_t *c_slot, uint64_t nc, const uint64_t *d_first,
                             const void *d_sub, const uint32_t *t_slot, uint64_t n, uint64_t key_base,
                             hipStream_t s);

// get on a store with target-kind containers, step 1: slot_of[i] (0xFFFFFFFF
// when absent), cnt[i] = pieces the digest expands into (1 for a chunk, the key
// count for a target), val[i] = the length it restores to.  d_res[0] += digests
// absent, d_res[3] += target-kind hits.
hipError_t launch_store_lookup_x(const IndexTable &t, const ScrubView &v, const uint8_t *d_digests, uint64_t n,
                                 uint32_t *slot_of, uint64_t *cnt, uint64_t *val, unsigned long long *d_res,
                                 hipStream_t s);

// step 2, after both scans (cnt -> first piece, val -> offset in d_out): the
// n_pieces pieces and their tile counts.
hipError_t launch_store_pieces_x(const IndexTable &t, const ScrubView &v, const uint64_t *loc, const uint8_t *arena,
                                 const uint32_t *slot_of, const uint64_t *pstart, const uint64_t *off, uint64_t n,
                                 uint64_t d_out, StorePiece *pieces, uint64_t *tiles, uint64_t n_pieces,
                                 hipStream_t s);

// spans[i] = {off[i], length of the digest's container}.
hipError_t launch_store_spans_x(const IndexTable &t, const uint32_t *slot_of, const uint64_t *off, uint64_t n,
                                void *d_spans, hipStream_t s);

// storage_iterator: per occupied slot, at its rank val[s] (the scanned flags):
// digest, kind, length, and its key count into key_first[rank].
hipError_t launch_store_iterate(const IndexTable &t, const ScrubView &v, const uint64_t *val, uint8_t *d_digests,
                                uint8_t *d_kinds, uint64_t *d_lengths, uint64_t *d_key_first, hipStream_t s);

// val[s] = keys of slot s (0 unless target-kind), for the scan that places them.
hipError_t launch_store_key_counts(const IndexTable &t, const ScrubView &v, uint64_t *val, hipStream_t s);
// The 32-byte keys (the target store's digests) of every target-kind slot, from
// d_keys + 32 * val[s] on.
hipError_t launch_store_keys(const IndexTable &t, const ScrubView &v, const uint64_t *val, uint8_t *d_keys,
                             hipStream_t s);

// ---- retain / collect ------------------------------------------------------------
// Keep the containers with refs[slot] > 0, drop the rest, slide the survivors
// down the arena in place (store_host.cpp store_retain; DESIGN.md "Removal and
// collection").  Survivors are numbered 0 .. m-1 in arena order.

// One move group: survivors [a, b), `bytes` padded bytes; direct = 1: copied
// arena -> arena in one launch, 0: gathered into the bounce buffer and written
// back with one device copy.
struct RetainGroup {
    uint64_t a, b, bytes, direct;
};

// refs[slot] += 1 for each of the n digests found (refs: slots u64, zeroed by
// the caller); d_res[0] += digests absent.
hipError_t launch_retain_refs(const IndexTable &t, const uint8_t *d_digests, uint64_t n, unsigned long long *refs,
                              unsigned long long *d_res, hipStream_t s);

// val[s] = 1 for the occupied slots with refs > 0, scanned in place (*d_total =
// m).  d_acc (zeroed): [0] sum of refs, [1] sum of refs * length, [2] bytes of
// the survivors, [3] their longest padded length.
hipError_t launch_retain_flag(const IndexTable &t, const unsigned long long *refs, uint64_t *val,
                              uint64_t *block_sums, unsigned long long *d_acc, unsigned long long *d_total,
                              hipStream_t s);

// The survivors in slot order: key[j] = arena offset | (length > 0), slot[j].
hipError_t launch_retain_list(const IndexTable &t, const uint64_t *loc, const unsigned long long *refs,
                              const uint64_t *val, uint64_t *key, uint32_t *slot, hipStream_t s);

// rocPRIM's stable radix sort of the pairs over key bits [0, end_bit).  temp ==
// NULL: *temp_bytes receives the scratch size and nothing runs.
hipError_t launch_retain_sort(void *temp, size_t *temp_bytes, const uint64_t *key_in, uint64_t *key_out,
                              const uint32_t *slot_in, uint32_t *slot_out, uint64_t m, unsigned end_bit,
                              hipStream_t s);

// In sorted order: newloc[0 .. m] = exclusive scan of round_up(length, 16)
// (newloc[m] = the arena bytes in use afterwards), the digests and {0, length}
// records the index insert takes.  block_sums: store_scan_blocks(m) + 1.
hipError_t launch_retain_layout(const IndexTable &t, const uint32_t *slot, uint64_t m, uint64_t *newloc,
                                uint64_t *block_sums, uint8_t *d_digests, void *d_chunks, hipStream_t s);

// The move groups, planned by one thread with binary searches over newloc.  The
// bounce buffer is W = max(max_pad, min(w_req, bytes to move)) bytes, max_pad
// being the longest padded length.  d_out: [0] groups, [1] direct, [2] bounced,
// [3] bytes moved, [4] != 0: the plan did not fit cap, [5] W, [6] the new offset
// of the first moved byte, [7] newloc[m].
hipError_t launch_retain_plan(const uint64_t *key, const uint64_t *newloc, uint64_t m, uint64_t w_req,
                              uint64_t max_pad, RetainGroup *groups, uint64_t cap, unsigned long long *d_out,
                              hipStream_t s);

// The piece list of all groups and, per group, a tile scan from 0: group g is
// moved by launch_store_copy(pieces + a, trel + a, b - a, ..., gtiles + g).
// tstart: m + 1; trel: m; gtiles: ng; block_sums: store_scan_blocks(m) + 1.
hipError_t launch_retain_pieces(const uint64_t *key, const uint64_t *newloc, uint64_t m, const RetainGroup *groups,
                                uint64_t ng, const uint8_t *arena, const uint8_t *bounce, StorePiece *pieces,
                                uint64_t *tstart, uint64_t *block_sums, uint64_t *trel, uint64_t *gtiles,
                                hipStream_t s);

// map[old slot] = new slot (map preset to 0xFF bytes), new_loc[new slot] = newloc.
hipError_t launch_retain_scatter(const uint32_t *old_slot, const uint32_t *new_slot, const uint64_t *newloc,
                                 uint64_t m, uint64_t *new_loc, uint32_t *map, hipStream_t s);

}  // namespace cdc
