// store_host.cpp -- C ABI of the device chunk store (include/chunkfs_amd.h,
// "Chunk store"): the reference's key -> data Database (src/system/database.rs:
// 10-36, 74-87), ChunkStorage::retrieve (src/system/storage.rs:141-157) and
// FileSystem::read_file_complete (src/system/mod.rs:149-160).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/chunkfs_amd.h"
#include "engine.hpp"
#include "index.hpp"
#include "store.hpp"
#include "store_internal.hpp"

struct cdc_store {
    int device = 0;
    cdc::IndexTable t{};
    uint64_t *loc = nullptr;       // [slots] arena offset of the slot's bytes
    uint8_t *arena = nullptr;
    uint64_t capacity = 0;         // unique digests accepted
    uint64_t arena_capacity = 0;
    uint64_t arena_used = 0;
    uint64_t *d_acc = nullptr;     // [12]: 0..4 index accumulators, 5 arena bytes taken, 8..11 precheck / lookup results
    uint32_t *d_pending = nullptr;
    // per-call scratch, grown to the largest n seen
    uint64_t n_cap = 0;
    uint32_t *d_slot = nullptr;          // [n_cap]
    uint8_t *d_new = nullptr;            // [n_cap]
    cdc::StorePiece *d_pieces = nullptr; // [n_cap]
    uint64_t *d_val = nullptr;           // [n_cap]
    uint64_t *d_tstart = nullptr;        // [n_cap]
    uint64_t *d_block = nullptr;         // [store_scan_blocks(n_cap) + 1]
    uint64_t s_cap = 0;
    uint64_t *d_streams = nullptr;       // [3 * s_cap + 1]: stream addresses, lens, first
    std::vector<uint64_t> h_streams;     // host image of d_streams
    hipStream_t stream = nullptr;
    cdc_index_stats_t st{};
    uint64_t epoch = 0;            // bumped by reset: locations resolved before it are stale
};

namespace {

#define ST_TRY(expr)                                                         \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            cdc::set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
            return CDC_EDEVICE;                                              \
        }                                                                    \
    } while (0)

int reset(cdc_store *st) {
    ST_TRY(hipSetDevice(st->device));
    ST_TRY(hipMemsetAsync(st->t.tag, 0, st->t.slots * 8, st->stream));
    ST_TRY(hipMemsetAsync(st->t.owner, 0xFF, st->t.slots * 8, st->stream));
    ST_TRY(hipStreamSynchronize(st->stream));
    st->st = cdc_index_stats_t{};
    st->arena_used = 0;
    ++st->epoch;
    return CDC_OK;
}

void free_scratch(cdc_store *st) {
    (void)hipFree(st->d_slot);
    (void)hipFree(st->d_new);
    (void)hipFree(st->d_pieces);
    (void)hipFree(st->d_val);
    (void)hipFree(st->d_tstart);
    (void)hipFree(st->d_block);
    st->d_slot = nullptr;
    st->d_new = nullptr;
    st->d_pieces = nullptr;
    st->d_val = st->d_tstart = st->d_block = nullptr;
    st->n_cap = 0;
}

void release(cdc_store *st) {
    (void)hipSetDevice(st->device);
    (void)hipFree(st->t.tag);
    (void)hipFree(st->t.digest);
    (void)hipFree(st->t.owner);
    (void)hipFree(st->t.length);
    (void)hipFree(st->loc);
    (void)hipFree(st->arena);
    (void)hipFree(st->d_acc);
    (void)hipFree(st->d_pending);
    (void)hipFree(st->d_streams);
    free_scratch(st);
    if (st->stream) (void)hipStreamDestroy(st->stream);
    delete st;
}

int create(int device, size_t max_chunks, size_t arena_bytes, cdc_store **out) {
    cdc_store *st = new cdc_store();
    st->device = device;
    st->capacity = max_chunks ? max_chunks : 1;
    st->arena_capacity = arena_bytes;
    uint64_t slots = 1024;
    while (slots < 2 * st->capacity) slots <<= 1;
    st->t.slots = slots;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
        delete st;
        cdc::set_error("no usable GPU for the chunk store");
        return CDC_EDEVICE;
    }
    auto fail = [&](hipError_t e) {
        cdc::set_error(std::string("chunk store allocation: ") + hipGetErrorString(e));
        release(st);
        return e == hipErrorOutOfMemory ? CDC_ENOMEM : CDC_EDEVICE;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail(e);
    if ((e = hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&st->t.tag, slots * 8)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&st->t.digest, slots * 32)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&st->t.owner, slots * 8)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&st->t.length, slots * 8)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&st->loc, slots * 8)) != hipSuccess) return fail(e);
    // Whole 16-byte blocks: the copy's aligned loads never leave the allocation.
    if ((e = hipMalloc(&st->arena, (arena_bytes / 16 + 1) * 16)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&st->d_acc, 12 * 8)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&st->d_pending, cdc::kIndexPendingCap * 4)) != hipSuccess) return fail(e);
    const int rc = reset(st);
    if (rc) {
        release(st);
        return rc;
    }
    *out = st;
    return CDC_OK;
}

// Scratch for a call over n chunks / digests.
int grow(cdc_store *st, uint64_t n) {
    if (st->n_cap >= n) return CDC_OK;
    free_scratch(st);
    const uint64_t cap = n + n / 8 + 64;
    ST_TRY(hipMalloc(&st->d_slot, cap * 4));
    ST_TRY(hipMalloc(&st->d_new, cap));
    ST_TRY(hipMalloc(&st->d_pieces, cap * sizeof(cdc::StorePiece)));
    ST_TRY(hipMalloc(&st->d_val, cap * 8));
    ST_TRY(hipMalloc(&st->d_tstart, cap * 8));
    ST_TRY(hipMalloc(&st->d_block, (cdc::store_scan_blocks(cap) + 1) * 8));
    st->n_cap = cap;
    return CDC_OK;
}

int64_t put(cdc_store *st, size_t n_streams, const uint8_t *const *d_streams, const uint64_t *lens,
            const uint64_t *first, const cdc_chunk_t *d_chunks, const uint8_t *d_digests, uint8_t *d_new,
            void *hip_stream) {
    const uint64_t n = first[n_streams];
    if (n == 0) return 0;
    if (!d_chunks || !d_digests) {
        cdc::set_error("chunk store put: NULL argument");
        return CDC_EINVAL;
    }
    if (n >= 0xFFFFFFFFull) {
        cdc::set_error("chunk store put: too many chunks in one call");
        return CDC_EINVAL;
    }
    ST_TRY(hipSetDevice(st->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : st->stream;
    int rc = grow(st, n);
    if (rc) return rc;
    if (st->s_cap < n_streams) {
        (void)hipFree(st->d_streams);
        st->d_streams = nullptr;
        st->s_cap = 0;
        ST_TRY(hipMalloc(&st->d_streams, (3 * n_streams + 1) * 8));
        st->s_cap = n_streams;
    }
    uint64_t *d_ptrs = st->d_streams, *d_lens = d_ptrs + n_streams, *d_first = d_lens + n_streams;
    st->h_streams.resize(3 * n_streams + 1);  // the store's own copy: outlives the upload whatever happens
    for (size_t i = 0; i < n_streams; ++i) {
        st->h_streams[i] = (uint64_t)(uintptr_t)d_streams[i];
        st->h_streams[n_streams + i] = lens[i];
    }
    memcpy(&st->h_streams[2 * n_streams], first, (n_streams + 1) * 8);
    ST_TRY(hipMemcpyAsync(d_ptrs, st->h_streams.data(), (3 * n_streams + 1) * 8, hipMemcpyHostToDevice, s));
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(st->d_acc);
    ST_TRY(hipMemsetAsync(st->d_acc, 0, 12 * 8, s));

    // The refusal rule: nothing below has touched the table or the arena yet.
    ST_TRY(cdc::launch_store_precheck(d_chunks, n, d_ptrs, d_lens, d_first, n_streams, st->d_pieces, acc + 8, s));
    uint64_t pre[4];  // out of bounds, padded bytes, tiles, wraps of the padded sum
    ST_TRY(hipMemcpyAsync(pre, st->d_acc + 8, sizeof pre, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    if (pre[0]) {
        cdc::set_error("chunk store put: " + std::to_string(pre[0]) + " chunk(s) reach outside their buffer");
        return CDC_EINVAL;
    }
    if (st->st.unique_chunks + n > st->capacity) {
        cdc::set_error("chunk store: max_chunks too small for this batch");
        return CDC_ENOMEM;
    }
    if (pre[3] || pre[1] > st->arena_capacity - st->arena_used) {
        // As if every chunk were new: the index's own rule.
        cdc::set_error("chunk store: arena too small for this batch");
        return CDC_ENOMEM;
    }

    uint8_t *flags = d_new ? d_new : st->d_new;
    ST_TRY(cdc::launch_index_insert(st->t, d_digests, d_chunks, n, st->st.chunks_written, st->d_slot,
                                    st->d_pending, flags, acc, s));
    ST_TRY(cdc::launch_store_compact(st->arena, st->arena_used, st->loc, st->d_slot, flags, st->d_pieces, n,
                                     st->d_val, st->d_tstart, st->d_block, pre[2], acc + 5, s));
    uint64_t res[6];  // the index's five, then the arena bytes the new chunks took
    ST_TRY(hipMemcpyAsync(res, st->d_acc, sizeof res, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    if (res[3] || res[4] > cdc::kIndexPendingCap) {
        cdc::set_error("chunk store: table full or too many 64-bit key collisions");
        return CDC_ENOMEM;
    }
    st->st.chunks_written += n;
    st->st.bytes_written += res[2];
    st->st.unique_chunks += res[0];
    st->st.unique_bytes += res[1];
    st->arena_used += res[5];
    return (int64_t)res[0];
}

}  // namespace

namespace cdc {

StoreView store_view(const cdc_store *st) {
    return StoreView{st->device, st->stream, st->epoch, st->t.slots, st->t.length, st->loc, st->arena, st->d_slot};
}

int64_t store_put_slots(cdc_store *st, const uint8_t *d_data, uint64_t data_len, const cdc_chunk_t *d_chunks,
                        const uint8_t *d_digests, uint64_t n, void *hip_stream) {
    const uint64_t lens[1] = {data_len}, first[2] = {0, n};
    const uint8_t *streams[1] = {d_data};
    return put(st, 1, streams, lens, first, d_chunks, d_digests, nullptr, hip_stream);
}

}  // namespace cdc

extern "C" {

int cdc_store_create(int device, size_t max_chunks, size_t arena_bytes, cdc_store_t **out) {
    if (!out) {
        cdc::set_error("cdc_store_create: out is NULL");
        return CDC_EINVAL;
    }
    *out = nullptr;
    return create(device, max_chunks, arena_bytes, out);
}

void cdc_store_destroy(cdc_store_t *st) {
    if (st) release(st);
}

int cdc_store_clear(cdc_store_t *st) {
    if (!st) {
        cdc::set_error("NULL store");
        return CDC_EINVAL;
    }
    return reset(st);
}

int cdc_store_stats(const cdc_store_t *st, cdc_store_stats_t *out) {
    if (!st || !out) {
        cdc::set_error("NULL argument");
        return CDC_EINVAL;
    }
    out->index = st->st;
    out->arena_capacity = st->arena_capacity;
    out->arena_used = st->arena_used;
    return CDC_OK;
}

int64_t cdc_store_put_device(cdc_store_t *st, const uint8_t *d_data, size_t data_len, const cdc_chunk_t *d_chunks,
                             const uint8_t *d_digests, size_t n, uint8_t *d_new, void *hip_stream) {
    if (!st) {
        cdc::set_error("NULL store");
        return CDC_EINVAL;
    }
    const uint64_t lens[1] = {data_len}, first[2] = {0, n};
    const uint8_t *streams[1] = {d_data};
    return put(st, 1, streams, lens, first, d_chunks, d_digests, d_new, hip_stream);
}

int64_t cdc_store_put_batch_device(cdc_store_t *st, size_t n_streams, const uint8_t *const *d_streams,
                                   const uint64_t *lens, const uint64_t *first, const cdc_chunk_t *d_chunks,
                                   const uint8_t *d_digests, uint8_t *d_new, void *hip_stream) {
    if (!st) {
        cdc::set_error("NULL store");
        return CDC_EINVAL;
    }
    if (n_streams == 0) return 0;
    if (!d_streams || !lens || !first) {
        cdc::set_error("cdc_store_put_batch_device: NULL argument");
        return CDC_EINVAL;
    }
    if (first[0] != 0) {
        cdc::set_error("cdc_store_put_batch_device: first[0] must be 0");
        return CDC_EINVAL;
    }
    for (size_t i = 0; i < n_streams; ++i)
        if (first[i + 1] < first[i]) {
            cdc::set_error("cdc_store_put_batch_device: first[] must not decrease");
            return CDC_EINVAL;
        }
    return put(st, n_streams, d_streams, lens, first, d_chunks, d_digests, d_new, hip_stream);
}

int64_t cdc_store_get_device(cdc_store_t *st, const uint8_t *d_digests, size_t n, uint8_t *d_out, size_t out_cap,
                             cdc_chunk_t *d_spans, void *hip_stream) {
    if (!st) {
        cdc::set_error("NULL store");
        return CDC_EINVAL;
    }
    if (n == 0) return 0;
    if (!d_digests || (out_cap && !d_out)) {
        cdc::set_error("cdc_store_get_device: NULL argument");
        return CDC_EINVAL;
    }
    ST_TRY(hipSetDevice(st->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : st->stream;
    const int rc = grow(st, n);
    if (rc) return rc;
    unsigned long long *res_d = reinterpret_cast<unsigned long long *>(st->d_acc) + 8;
    ST_TRY(hipMemsetAsync(res_d, 0, 3 * 8, s));
    ST_TRY(cdc::launch_store_lookup(st->t, st->loc, st->arena, d_digests, n, st->d_pieces, nullptr, res_d, s));
    ST_TRY(cdc::launch_store_plan_get(st->d_pieces, n, (uint64_t)(uintptr_t)d_out, st->d_val, st->d_tstart,
                                      st->d_block, res_d, s));
    uint64_t res[3];  // digests absent, total bytes, total tiles
    ST_TRY(hipMemcpyAsync(res, res_d, sizeof res, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    if (res[0]) {
        cdc::set_error("chunk store get: " + std::to_string(res[0]) + " digest(s) not found");
        return CDC_ENOTFOUND;
    }
    if (res[1] > out_cap) return (int64_t)res[1];  // sizes a read: nothing written
    ST_TRY(cdc::launch_store_gather(st->d_pieces, st->d_tstart, n, res[2], (uint64_t)(uintptr_t)d_out, d_spans, s));
    ST_TRY(hipStreamSynchronize(s));
    return (int64_t)res[1];
}

int64_t cdc_store_contains_device(cdc_store_t *st, const uint8_t *d_digests, size_t n, uint8_t *d_found,
                                  void *hip_stream) {
    if (!st) {
        cdc::set_error("NULL store");
        return CDC_EINVAL;
    }
    if (n == 0) return 0;
    if (!d_digests) {
        cdc::set_error("cdc_store_contains_device: NULL argument");
        return CDC_EINVAL;
    }
    ST_TRY(hipSetDevice(st->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : st->stream;
    const int rc = grow(st, n);
    if (rc) return rc;
    unsigned long long *res_d = reinterpret_cast<unsigned long long *>(st->d_acc) + 8;
    ST_TRY(hipMemsetAsync(res_d, 0, 3 * 8, s));
    ST_TRY(cdc::launch_store_lookup(st->t, st->loc, st->arena, d_digests, n, st->d_pieces, d_found, res_d, s));
    uint64_t missing = 0;
    ST_TRY(hipMemcpyAsync(&missing, res_d, 8, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    return (int64_t)(n - missing);
}

}  // extern "C"
