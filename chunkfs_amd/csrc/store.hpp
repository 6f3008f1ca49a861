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

}  // namespace cdc
