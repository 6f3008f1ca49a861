// pack.hpp -- kernels of cdc_file_pack_device and cdc_files_unpack_device
// (pack.hip; the host side is in files_host.cpp, the arithmetic in
// pack_plan.hpp): one file of the layer as a self-describing, deduplicated,
// deterministic byte image, built and consumed on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "files.hpp"
#include "index.hpp"
#include "pack_plan.hpp"
#include "store.hpp"

namespace cdc {

// ---- packing -------------------------------------------------------------------
// Steps (a) and (b) over the n > 0 spans of a file: per slot the file names, the
// first span that names it (firstpos, by atomicMin as the distribution does) and
// whether it is excluded (excl: a span of `since` names it -- since_slot / ns,
// nullable -- or a span i of the file with have[i] != 0 does; have nullable).
// excl / firstpos: table-sized scratch of which only the slots the file names
// are initialised.  rank[i] = 1 where span i is the first occurrence of a
// carried slot, poff[i] = round_up(its length, 16) there; both scanned in place
// (bs_rank / bs_off: store_scan_blocks(n) + 1 each).  h_out (pinned): [0] =
// carried chunks, [1] = bytes of the data section.  d_acc (device, two words,
// zeroed here): [0] += spans whose slot is excluded, [1] += unpadded bytes of
// the carried chunks.
hipError_t launch_pack_mark(const SpanTable &t, uint64_t n, const uint32_t *since_slot, uint64_t ns,
                            const uint8_t *have, uint64_t slots, uint32_t *excl, uint64_t *firstpos, uint64_t *rank,
                            uint64_t *poff, uint64_t *bs_rank, uint64_t *bs_off, unsigned long long *d_acc,
                            unsigned long long *h_out, hipStream_t s);

// Steps (c) and (d) once the host has the sizes: one kernel writes the header,
// the five index sections and every padding byte, and leaves the piece list of
// the carried chunks (arena -> data section) for the store's copy.  pieces /
// tstart: n_chunks entries; block_sums: store_scan_blocks(n_chunks) + 1.  n may
// be 0 (the tables are not touched then).
hipError_t launch_pack_write(const SpanTable &t, uint64_t n, const uint32_t *excl, const uint64_t *firstpos,
                             const uint64_t *rank, const uint64_t *poff, const PackHeader &h, const PackLayout &l,
                             uint8_t *d_pack, uint64_t arena, StorePiece *pieces, uint64_t *tstart,
                             uint64_t *block_sums, hipStream_t s);

// ---- unpacking -----------------------------------------------------------------
// What the validation and the lookup leave, device words; the host presets
// count[] and the sums to 0 and first[] to ~0 (pack_result_preset).
struct PackResult {
    unsigned long long count[kPackChecks];  // failures per check
    unsigned long long first[kPackChecks];  // the smallest offending index
    unsigned long long sum_low, sum_wraps;  // the span lengths
    unsigned long long externals;           // spans with span_chunk == ~0
    unsigned long long missing, missing_first;    // external spans whose digest the store does not hold
    unsigned long long mislen, mislen_first;      // external spans whose stored chunk has another length
    unsigned long long mismatch, mismatch_first;  // carried chunks whose SHA-256 is not their digest
};
hipError_t pack_result_preset(PackResult *d_res, hipStream_t s);

// The validation kernel over a pack whose header passed pack_check_header: the
// per-index predicates of pack_plan.hpp, the length sum and the external count.
hipError_t launch_pack_validate(const PackView &v, PackResult *d_res, hipStream_t s);

// slot[i] = the table slot that holds span i's digest, 0xFFFFFFFF when the store
// does not hold it; for the external spans the missing and wrong-length counts.
// Reads the digests, lengths and span_chunk at [0, n_spans) only.
hipError_t launch_pack_lookup(const IndexTable &t, const PackView &v, uint32_t *slot, PackResult *d_res,
                              hipStream_t s);

// After the validation: the carried chunks as a put takes them.  chunks[k] =
// {chunk_off[k], length}, digests[k] = the digest of the chunk's first span.
hipError_t launch_pack_gather(const PackView &v, void *d_chunks, uint8_t *d_digests, hipStream_t s);

// mismatch += chunks k with sha[k] != digests[k]; mismatch_first = the smallest.
hipError_t launch_pack_verify(const uint8_t *sha, const uint8_t *digests, uint64_t n_chunks, PackResult *d_res,
                              hipStream_t s);

// After the put of the carried chunks: slot[i] = slot_of[span_chunk[i]] for the
// spans the pack carries; the external spans keep the lookup's slot.
hipError_t launch_pack_slots(const PackView &v, const uint32_t *slot_of, uint32_t *slot, hipStream_t s);

}  // namespace cdc
