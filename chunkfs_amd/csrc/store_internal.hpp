// store_internal.hpp -- what the file layer (files_host.cpp) needs from the
// chunk store's host object (store_host.cpp) beyond the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/chunkfs_amd.h"
#include "host_common.hpp"
#include "store.hpp"

namespace cdc {

// A snapshot of the store's device arrays.  epoch counts the clears: a table
// slot or arena offset resolved under another epoch is stale.  slot_of is the
// per-chunk slot list of the last put (launch_index_insert's d_slot_of,
// duplicates included), valid until the next call on the store.
struct StoreView {
    int device;
    hipStream_t stream;
    uint64_t epoch;
    uint64_t slots;
    const uint64_t *length;  // [slots] length of the slot's chunk
    const uint64_t *loc;     // [slots] arena offset of the slot's bytes
    const uint8_t *arena;
    const uint32_t *slot_of;
};

StoreView store_view(const cdc_store *st);

// The store's index table, for a lookup that answers with the slot
// (cdc_files_unpack_device, pack.hip).
IndexTable store_index(const cdc_store *st);

// Counts `chunks` inserts of `bytes` bytes in all whose digests the store held
// already: what a put of them would add to chunks_written and bytes_written,
// and nothing else.  An unpack puts each carried chunk once; the file's other
// spans are such inserts.
void store_count_written(cdc_store *st, uint64_t chunks, uint64_t bytes);

// cdc_store_put_device without the new flags; on success store_view().slot_of
// holds the n slots.  Same checks, same refusal rule, same return value.
int64_t store_put_slots(cdc_store *st, const uint8_t *d_data, uint64_t data_len, const cdc_chunk_t *d_chunks,
                        const uint8_t *d_digests, uint64_t n, void *hip_stream);

// cdc_store_put_batch_device in the same way: first[] (HOST, n_streams + 1
// entries, first[0] = 0, not decreasing) is the caller's to get right; on
// success store_view().slot_of holds the first[n_streams] slots in chunk order.
int64_t store_put_batch_slots(cdc_store *st, size_t n_streams, const uint8_t *const *d_streams, const uint64_t *lens,
                              const uint64_t *first, const cdc_chunk_t *d_chunks, const uint8_t *d_digests,
                              void *hip_stream);

// The scrubbed state: true once the store holds target-kind containers, whose
// bytes are found through the slot's current container (the base arena was
// reset by the scrub, so a location cached before it is stale).  *stale: the
// target store was cleared since; a read that needs a target-kind container
// must return CDC_ENOTFOUND.
bool store_scrub_view(const cdc_store *st, ScrubView *view, bool *stale);

// Retain by per-slot reference counts, the one primitive behind
// cdc_files_collect and cdc_store_retain_device (the contract: chunkfs_amd.h
// "Removal and collection").  d_refs: DEVICE u64[slots]; a container stays iff
// its slot is occupied and refs > 0.  d_map (DEVICE u32[slots], nullable)
// receives old slot -> new slot, 0xFFFFFFFF for a dropped or empty slot; the new
// offsets are store_view().loc afterwards.  *out is always filled on success.
// Every refusal and every allocation comes before the first write to the table
// or the arena; a CDC_EDEVICE after that leaves the store fit only for clear or
// destroy.
int store_retain(cdc_store *st, const unsigned long long *d_refs, uint32_t *d_map, cdc_collect_stats_t *out,
                 hipStream_t s);

// cdc_debug_collect_split's six figures of this thread: store_retain fills
// [0..4] and zeroes [5], the file layer sets [5].
double *collect_split();

// Device memory of one call, freed when the call returns.
struct DeviceScratch {
    std::vector<void *> ptrs;
    ~DeviceScratch() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    hipError_t alloc(T **out, uint64_t count) {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(p);
        *out = static_cast<T *>(p);
        return e;
    }
};

// Per-item scratch and the two arrays of the scan over it.
template <typename T>
struct ScanScratch {
    uint64_t cap = 0;
    DeviceBuf<T> items;
    DeviceBuf<uint64_t> val, block;  // [cap], [store_scan_blocks(cap) + 1]
    hipError_t grow(uint64_t n) {
        const uint64_t c = n + n / 8 + 64;
        return grow_group(cap, n, c, items, c, val, c, block, store_scan_blocks(c) + 1);
    }
};

// The device a chunker handle is bound to (capi.cpp).
int handle_device(const cdc_handle *h);
// The longest chunk its rule cuts (capi.cpp): the splice's trust window.
uint64_t handle_max_chunk(const cdc_handle *h);

}  // namespace cdc
