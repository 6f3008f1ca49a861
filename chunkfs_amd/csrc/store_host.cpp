// store_host.cpp -- C ABI of the device chunk store (include/chunkfs_amd.h,
// "Chunk store"): the reference's key -> data Database (src/system/database.rs:
// 10-36, 74-87), ChunkStorage::retrieve (src/system/storage.rs:141-157) and
// FileSystem::read_file_complete (src/system/mod.rs:149-160); and of the scrub
// stage ("Scrub stage"): the target map as a second store, the Scrub hook
// (src/system/scrub.rs), DataContainer kinds with resolved key runs
// (storage.rs:12-21), new_with_scrubber / scrub / iterator (storage.rs:165-235).
// Retain / collect ("Removal and collection") is this project's own.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/chunkfs_amd.h"
#include "../../include/chunkfs_amd_debug.h"
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
    // per-call scratch, grown to the largest n seen; n_cap is 0 after a growth that failed
    uint64_t n_cap = 0;
    cdc::DeviceBuf<uint32_t> d_slot;           // [n_cap]
    cdc::DeviceBuf<uint8_t> d_new;             // [n_cap]
    cdc::DeviceBuf<cdc::StorePiece> d_pieces;  // [n_cap]
    cdc::DeviceBuf<uint64_t> d_val, d_tstart;  // [n_cap]
    cdc::DeviceBuf<uint64_t> d_block;          // [store_scan_blocks(n_cap) + 1]
    cdc::DeviceBuf<uint64_t> d_streams;        // [3 * n_streams + 1]: stream addresses, lens, first
    std::vector<uint64_t> h_streams;     // host image of d_streams
    hipStream_t stream = nullptr;
    cdc_index_stats_t st{};
    uint64_t epoch = 0;            // bumped by reset: locations resolved before it are stale
    // Scrub stage (allocated by cdc_store_set_target): the target map and this
    // store's containers that have become lists of its keys.
    cdc_store *target = nullptr;   // not owned
    uint64_t target_epoch = 0;     // the target's epoch the keys were resolved under
    cdc::ScrubState sc{};          // kind / key_first / key_count: [slots]; key_slot / key_off: [key_cap]
    uint64_t key_cap = 0, keys_used = 0;
    uint64_t target_containers = 0;
    uint64_t scrubbed_bytes = 0;   // unique bytes whose containers are target-kind now
    cdc::ScanScratch<cdc::StorePiece> x;  // get through targets: per piece, with the tile counts
    // The hasher of every digest in the table (CDC_HASH_*): the file layer and
    // the re-chunk scrub hash with it; nothing else here reads digests' origin.
    int hash = CDC_HASH_SHA256;
    bool is_target = false;        // some store has been given this one as its target
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
    if (st->sc.kind) ST_TRY(hipMemsetAsync(st->sc.kind, 0, st->t.slots, st->stream));
    ST_TRY(hipStreamSynchronize(st->stream));
    st->st = cdc_index_stats_t{};
    st->arena_used = 0;
    ++st->epoch;
    // The containers and their keys are gone; the attachment stays and follows
    // the target as it is now.
    st->keys_used = st->target_containers = st->scrubbed_bytes = 0;
    if (st->target) st->target_epoch = st->target->epoch;
    return CDC_OK;
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
    (void)hipFree(st->sc.kind);
    (void)hipFree(st->sc.key_first);
    (void)hipFree(st->sc.key_count);
    (void)hipFree(st->sc.key_slot);
    (void)hipFree(st->sc.key_off);
    if (st->stream) (void)hipStreamDestroy(st->stream);
    delete st;  // the per-call scratch goes with it, the device still current
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
    const uint64_t cap = n + n / 8 + 64;
    ST_TRY(cdc::grow_group(st->n_cap, n, cap, st->d_slot, cap, st->d_new, cap, st->d_pieces, cap, st->d_val, cap,
                           st->d_tstart, cap, st->d_block, cdc::store_scan_blocks(cap) + 1));
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
    ST_TRY(st->d_streams.room(3 * n_streams + 1));
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

// ---- scrub stage -------------------------------------------------------------------
cdc::ScrubView scrub_view(const cdc_store *st) {
    const cdc_store *t = st->target;
    return cdc::ScrubView{st->sc.kind, st->sc.key_first, st->sc.key_count, st->sc.key_slot, st->sc.key_off,
                          t ? t->t.length : nullptr, t ? t->loc : nullptr, t ? t->t.digest : nullptr,
                          t ? (uint64_t)(uintptr_t)t->arena : 0};
}

// The keys were resolved in a target that has been cleared since.
bool target_stale(const cdc_store *st) {
    return st->target && st->target_containers && st->target->epoch != st->target_epoch;
}

// Room for `need` keys; the run arrays keep their contents.
int reserve_keys(cdc_store *st, uint64_t need, hipStream_t s) {
    if (need <= st->key_cap) return CDC_OK;
    uint64_t cap = st->key_cap ? st->key_cap : 1024;
    while (cap < need) cap *= 2;
    uint32_t *slot = nullptr;
    uint64_t *off = nullptr;
    hipError_t e = hipMalloc(&slot, cap * 4);
    if (e == hipSuccess) e = hipMalloc(&off, cap * 8);
    if (e == hipSuccess && st->keys_used) {
        e = hipMemcpyAsync(slot, st->sc.key_slot, st->keys_used * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(off, st->sc.key_off, st->keys_used * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) {
        (void)hipFree(slot);
        (void)hipFree(off);
        cdc::set_error(std::string("chunk store scrub: key array growth: ") + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? CDC_ENOMEM : CDC_EDEVICE;
    }
    (void)hipFree(st->sc.key_slot);
    (void)hipFree(st->sc.key_off);
    st->sc.key_slot = slot;
    st->sc.key_off = off;
    st->key_cap = cap;
    return CDC_OK;
}

// Containers and bytes of one RECHUNK group: CHUNKFS_AMD_SCRUB_GROUP=containers[,bytes].
void scrub_group_limits(uint64_t *containers, uint64_t *bytes) {
    *containers = 1u << 20;  // measured on a 1 GiB store (DESIGN.md "Scrub stage"): fewer, larger groups win,
    *bytes = 1ull << 30;     // and a store that fits one group is chunked once instead of twice
    if (const char *v = std::getenv("CHUNKFS_AMD_SCRUB_GROUP")) {
        unsigned long long a = 0, b = 0;
        const int got = std::sscanf(v, "%llu,%llu", &a, &b);
        if (got >= 1 && a >= 1) *containers = a;
        if (got >= 2 && b >= 1) *bytes = b;
    }
}

int set_target(cdc_store *st, cdc_store *target) {
    if (!st || !target) {
        cdc::set_error("cdc_store_set_target: NULL store");
        return CDC_EINVAL;
    }
    if (st == target) {
        cdc::set_error("cdc_store_set_target: a store cannot be its own target");
        return CDC_EINVAL;
    }
    if (st->device != target->device) {
        cdc::set_error("cdc_store_set_target: the two stores are on different devices");
        return CDC_EINVAL;
    }
    if (target->target) {
        cdc::set_error("cdc_store_set_target: the target store has a target itself");
        return CDC_EINVAL;
    }
    if (st->target_containers) {
        cdc::set_error("cdc_store_set_target: the store holds containers that refer to its present target");
        return CDC_EINVAL;
    }
    if (st->hash != target->hash) {
        cdc::set_error("cdc_store_set_target: the two stores have different hashers (cdc_store_set_hash)");
        return CDC_EINVAL;
    }
    ST_TRY(hipSetDevice(st->device));
    if (!st->sc.kind) {
        cdc::ScrubState sc{};
        hipError_t e = hipMalloc(&sc.kind, st->t.slots);
        if (e == hipSuccess) e = hipMalloc(&sc.key_first, st->t.slots * 8);
        if (e == hipSuccess) e = hipMalloc(&sc.key_count, st->t.slots * 4);
        if (e == hipSuccess) e = hipMemsetAsync(sc.kind, 0, st->t.slots, st->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(st->stream);
        if (e != hipSuccess) {
            (void)hipFree(sc.kind);
            (void)hipFree(sc.key_first);
            (void)hipFree(sc.key_count);
            cdc::set_error(std::string("cdc_store_set_target: ") + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? CDC_ENOMEM : CDC_EDEVICE;
        }
        st->sc = sc;
    }
    st->target = target;
    st->target_epoch = target->epoch;
    target->is_target = true;
    return CDC_OK;
}

int scrub(cdc_store *st, int scrubber, cdc_handle_t *chunker, cdc_scrub_measurements_t *out, void *hip_stream) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!st || !out) {
        cdc::set_error("cdc_store_scrub: NULL argument");
        return CDC_EINVAL;
    }
    if (!st->target) {
        cdc::set_error("cdc_store_scrub: no target store attached (this store was created without a scrubber)");
        return CDC_EINVAL;
    }
    if (scrubber != CDC_SCRUB_DUMB && scrubber != CDC_SCRUB_COPY && scrubber != CDC_SCRUB_RECHUNK) {
        cdc::set_error("cdc_store_scrub: unknown scrubber");
        return CDC_EINVAL;
    }
    if (scrubber == CDC_SCRUB_RECHUNK && (!chunker || cdc::handle_device(chunker) != st->device)) {
        cdc::set_error("cdc_store_scrub: RECHUNK needs a chunker on the store's device");
        return CDC_EINVAL;
    }
    *out = cdc_scrub_measurements_t{0, 0.0, 0};
    if (scrubber == CDC_SCRUB_DUMB) return CDC_OK;  // scrub.rs:116-129
    cdc_store *tg = st->target;
    if (tg->epoch != st->target_epoch) {
        if (st->target_containers) {
            cdc::set_error("chunk store scrub: the target store was cleared; clear this store too");
            return CDC_ENOTFOUND;
        }
        st->target_epoch = tg->epoch;
    }
    ST_TRY(hipSetDevice(st->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : st->stream;
    auto finish = [&](uint64_t processed) {
        out->processed_data = processed;
        out->running_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return CDC_OK;
    };
    // No chunk-kind container (an empty store, or nothing written since the last
    // scrub): nothing to list, and no kernel is launched over zero items.
    if (st->st.unique_chunks == st->target_containers) return finish(0);

    // 1. The chunk-kind containers, in slot order.
    cdc::DeviceScratch mem;
    const uint64_t slots = st->t.slots;
    uint64_t *val = nullptr, *block = nullptr;
    ST_TRY(mem.alloc(&val, slots));
    ST_TRY(mem.alloc(&block, cdc::store_scan_blocks(slots) + 1));
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(st->d_acc) + 8;
    ST_TRY(hipMemsetAsync(acc, 0, 4 * 8, s));
    ST_TRY(cdc::launch_scrub_flag(st->t, st->sc.kind, 0, val, block, acc, s));
    uint64_t nc = 0;
    ST_TRY(hipMemcpyAsync(&nc, acc, 8, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    if (nc == 0) return finish(0);
    cdc_chunk_t *c_chunks = nullptr;
    uint8_t *c_dig = nullptr;
    uint32_t *c_slot = nullptr;
    ST_TRY(mem.alloc(&c_chunks, nc));
    ST_TRY(mem.alloc(&c_dig, nc * 32));
    ST_TRY(mem.alloc(&c_slot, nc));
    ST_TRY(cdc::launch_scrub_list(st->t, st->sc.kind, st->loc, val, c_chunks, c_dig, c_slot, acc + 1, s));
    uint64_t processed = 0;
    ST_TRY(hipMemcpyAsync(&processed, acc + 1, 8, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));

    auto converted = [&](uint64_t containers, uint64_t bytes, uint64_t keys) {
        st->target_containers += containers;
        st->scrubbed_bytes += bytes;
        st->keys_used += keys;
    };

    if (scrubber == CDC_SCRUB_COPY) {
        // 2. scrub.rs:85-114: target.insert(hash, chunk) with the base arena as
        // the source -- the digest is the key, nothing is hashed again.  The
        // put's own precheck is the planning pass: it refuses before it writes.
        int rc = reserve_keys(st, st->keys_used + nc, s);
        if (rc) return rc;
        const uint64_t lens[1] = {st->arena_used}, first[2] = {0, nc};
        const uint8_t *streams[1] = {st->arena};
        const int64_t got = put(tg, 1, streams, lens, first, c_chunks, c_dig, nullptr, s);
        if (got < 0) return (int)got;
        ST_TRY(cdc::launch_scrub_mark(st->sc, c_slot, nc, nullptr, nullptr, tg->d_slot, nc, st->keys_used, s));
        ST_TRY(hipStreamSynchronize(s));
        converted(nc, processed, nc);
        st->arena_used = 0;  // every chunk container was converted: no byte of the arena is live
        return finish(processed);
    }

    // 3. RECHUNK: every container is one stream of a batch; groups bound the scratch.
    std::vector<cdc_chunk_t> h_c(nc);
    ST_TRY(hipMemcpyAsync(h_c.data(), c_chunks, nc * sizeof(cdc_chunk_t), hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    uint64_t g_containers, g_bytes;
    scrub_group_limits(&g_containers, &g_bytes);
    std::vector<uint64_t> gstart{0};  // group g = containers [gstart[g], gstart[g + 1])
    {
        uint64_t cnt = 0, bytes = 0;
        for (uint64_t j = 0; j < nc; ++j) {
            if (cnt && (cnt >= g_containers || bytes + h_c[j].length > g_bytes)) {
                gstart.push_back(j);
                cnt = bytes = 0;
            }
            ++cnt;
            bytes += h_c[j].length;
        }
        gstart.push_back(nc);
    }
    const uint64_t groups = gstart.size() - 1;
    std::vector<const uint8_t *> ptrs(nc);
    std::vector<uint64_t> lens(nc);
    uint64_t sub_cap = 0, max_group = 0;
    for (uint64_t j = 0; j < nc; ++j) {
        ptrs[j] = st->arena + h_c[j].offset;  // 16-byte aligned by the store's layout
        lens[j] = h_c[j].length;
    }
    for (uint64_t g = 0; g < groups; ++g) {
        const uint64_t a = gstart[g], ng = gstart[g + 1] - a;
        const uint64_t cap = cdc_batch_max_chunks(chunker, ng, &lens[a]);
        sub_cap = cap > sub_cap ? cap : sub_cap;
        max_group = ng > max_group ? ng : max_group;
    }
    cdc_chunk_t *d_sub = nullptr;
    uint8_t *d_dig = nullptr;
    uint64_t *d_first = nullptr;
    ST_TRY(mem.alloc(&d_sub, sub_cap));
    ST_TRY(mem.alloc(&d_dig, sub_cap * 32));
    ST_TRY(mem.alloc(&d_first, max_group + 1));
    std::vector<uint64_t> first(max_group + 1);
    auto chunk_group = [&](uint64_t g) -> int64_t {
        const uint64_t a = gstart[g], ng = gstart[g + 1] - a;
        return cdc_chunk_batch_device(chunker, ng, &ptrs[a], &lens[a], d_sub, sub_cap, first.data(), s);
    };

    // The planning pass: key count and padded bytes "as if every key were new",
    // before the target or this store is touched.  One group needs none: the
    // put's own precheck refuses before it writes, and the lists are kept.
    if (groups > 1) {
        uint64_t keys = 0;
        ST_TRY(hipMemsetAsync(acc + 2, 0, 8, s));
        for (uint64_t g = 0; g < groups; ++g) {
            const int64_t n = chunk_group(g);
            if (n < 0) return (int)n;
            keys += (uint64_t)n;
            ST_TRY(cdc::launch_scrub_padsum(d_sub, (uint64_t)n, acc + 2, s));
        }
        uint64_t padded = 0;
        ST_TRY(hipMemcpyAsync(&padded, acc + 2, 8, hipMemcpyDeviceToHost, s));
        ST_TRY(hipStreamSynchronize(s));
        if (tg->st.unique_chunks + keys > tg->capacity) {
            cdc::set_error("chunk store scrub: the target's max_chunks is too small for the sub-chunks");
            return CDC_ENOMEM;
        }
        if (padded > tg->arena_capacity - tg->arena_used) {
            cdc::set_error("chunk store scrub: the target's arena is too small for the sub-chunks");
            return CDC_ENOMEM;
        }
        const int rc = reserve_keys(st, st->keys_used + keys, s);
        if (rc) return rc;
    }
    uint64_t done_bytes = 0;
    for (uint64_t g = 0; g < groups; ++g) {
        const uint64_t a = gstart[g], ng = gstart[g + 1] - a;
        const int64_t n = chunk_group(g);
        if (n < 0) return (int)n;
        int rc = cdc_hash_batch_device(chunker, st->hash, ng, &ptrs[a], first.data(), d_sub, d_dig, s);
        if (rc) return rc;
        if (groups == 1 && (rc = reserve_keys(st, st->keys_used + (uint64_t)n, s)) != CDC_OK) return rc;
        const int64_t got = put(tg, ng, &ptrs[a], &lens[a], first.data(), d_sub, d_dig, nullptr, s);
        if (got < 0) return (int)got;  // one group: nothing was touched; later groups: the index's own errors only
        ST_TRY(hipMemcpyAsync(d_first, first.data(), (ng + 1) * 8, hipMemcpyHostToDevice, s));
        ST_TRY(cdc::launch_scrub_mark(st->sc, c_slot + a, ng, d_first, d_sub, tg->d_slot, (uint64_t)n, st->keys_used, s));
        ST_TRY(hipStreamSynchronize(s));
        uint64_t bytes = 0;
        for (uint64_t j = a; j < a + ng; ++j) bytes += lens[j];
        converted(ng, bytes, (uint64_t)n);
        done_bytes += bytes;
    }
    st->arena_used = 0;
    return finish(done_bytes);
}

// Flags over the slots -> ranks; returns the scratch through mem.
int rank_slots(cdc_store *st, cdc::DeviceScratch &mem, int want_kind, uint64_t **val, uint64_t *total, hipStream_t s) {
    uint64_t *block = nullptr;
    ST_TRY(mem.alloc(val, st->t.slots));
    ST_TRY(mem.alloc(&block, cdc::store_scan_blocks(st->t.slots) + 1));
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(st->d_acc) + 8;
    ST_TRY(cdc::launch_scrub_flag(st->t, st->sc.kind, want_kind, *val, block, acc, s));
    ST_TRY(hipMemcpyAsync(total, acc, 8, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    return CDC_OK;
}

// cdc_store_get_device once target-kind containers exist: a digest expands
// into its keys' pieces.
int64_t get_expanded(cdc_store *st, const uint8_t *d_digests, size_t n, uint8_t *d_out, size_t out_cap,
                     cdc_chunk_t *d_spans, hipStream_t s) {
    const cdc::ScrubView v = scrub_view(st);
    unsigned long long *res_d = reinterpret_cast<unsigned long long *>(st->d_acc) + 8;
    ST_TRY(hipMemsetAsync(res_d, 0, 4 * 8, s));
    ST_TRY(cdc::launch_store_lookup_x(st->t, v, d_digests, n, st->d_slot, st->d_tstart, st->d_val, res_d, s));
    ST_TRY(cdc::launch_store_scan(st->d_tstart, n, st->d_block, res_d + 2, s));  // first piece of each digest
    ST_TRY(cdc::launch_store_scan(st->d_val, n, st->d_block, res_d + 1, s));     // its offset in d_out
    uint64_t res[4];  // digests absent, total bytes, total pieces, target-kind hits
    ST_TRY(hipMemcpyAsync(res, res_d, sizeof res, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    if (res[0]) {
        cdc::set_error("chunk store get: " + std::to_string(res[0]) + " digest(s) not found");
        return CDC_ENOTFOUND;
    }
    if (res[3] && target_stale(st)) {
        cdc::set_error("chunk store get: the target store was cleared since these containers were scrubbed");
        return CDC_ENOTFOUND;
    }
    if (res[1] > out_cap) return (int64_t)res[1];
    const uint64_t np = res[2];
    ST_TRY(st->x.grow(np));
    if (np) {
        ST_TRY(cdc::launch_store_pieces_x(st->t, v, st->loc, st->arena, st->d_slot, st->d_tstart, st->d_val, n,
                                          (uint64_t)(uintptr_t)d_out, st->x.items, st->x.val, np, s));
        ST_TRY(cdc::launch_store_scan(st->x.val, np, st->x.block, nullptr, s));
        // A piece adds at most two ragged tiles to its whole ones; the exact total is read on the device.
        ST_TRY(cdc::launch_store_copy(st->x.items, st->x.val, np, res[1] / cdc::kStoreTile + 2 * np,
                                      st->x.block + cdc::store_scan_blocks(np), s));
    }
    if (d_spans) ST_TRY(cdc::launch_store_spans_x(st->t, st->d_slot, st->d_val, n, d_spans, s));
    ST_TRY(hipStreamSynchronize(s));
    return (int64_t)res[1];
}

// ---- retain / collect ---------------------------------------------------------------
// Bytes of the bounce buffer before it is clipped to the bytes to move and raised
// to the longest container: CHUNKFS_AMD_GC_BOUNCE=bytes.
uint64_t retain_bounce_request() {
    if (const char *v = std::getenv("CHUNKFS_AMD_GC_BOUNCE")) {
        char *end = nullptr;
        const unsigned long long w = std::strtoull(v, &end, 10);
        if (end != v) return w;
    }
    return 256ull << 20;
}

// An allocation that fails is a refusal (CDC_ENOMEM), not a device error.
#define ST_ALLOC(expr)                                                                        \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (void)hipGetLastError();                                                          \
            cdc::set_error(std::string("chunk store collect: ") + #expr + ": " + hipGetErrorString(e_)); \
            return e_ == hipErrorOutOfMemory ? CDC_ENOMEM : CDC_EDEVICE;                      \
        }                                                                                     \
    } while (0)

// The second set of table arrays the survivors are inserted into; freed unless adopted.
struct NewTable {
    cdc::IndexTable t{};
    uint64_t *loc = nullptr;
    ~NewTable() {
        (void)hipFree(t.tag);
        (void)hipFree(t.digest);
        (void)hipFree(t.owner);
        (void)hipFree(t.length);
        (void)hipFree(loc);
    }
};

int retain(cdc_store *st, const unsigned long long *d_refs, uint32_t *d_map, cdc_collect_stats_t *out,
           hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    auto last = t0;
    double split[6] = {0, 0, 0, 0, 0, 0};  // cdc_debug_collect_split
    auto lap = [&](int phase) {
        const auto now = std::chrono::steady_clock::now();
        split[phase] += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    };
    if (st->target_containers) {
        cdc::set_error("chunk store collect: the store holds target-kind containers (scrubbed); not supported");
        return CDC_ENOTSUP;
    }
    ST_TRY(hipSetDevice(st->device));
    const uint64_t slots = st->t.slots;
    cdc::DeviceScratch mem;

    // 1. Which containers stay, how many, and the totals the stats are set from.
    uint64_t *val = nullptr, *block = nullptr;
    unsigned long long *acc = nullptr;  // [0..3] the flag pass, [4] m, [8..12] the insert, [16..23] the plan
    ST_ALLOC(mem.alloc(&val, slots));
    ST_ALLOC(mem.alloc(&block, cdc::store_scan_blocks(slots) + 1));
    ST_ALLOC(mem.alloc(&acc, 24));
    ST_TRY(hipMemsetAsync(acc, 0, 24 * 8, s));
    ST_TRY(cdc::launch_retain_flag(st->t, d_refs, val, block, acc, acc + 4, s));
    uint64_t h[5];  // sum of refs, sum of refs * length, survivors' bytes, longest padded length, m
    ST_TRY(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    const uint64_t m = h[4];
    lap(0);
    // Owners are renumbered 0 .. m-1 and the next put's base is chunks_written =
    // the sum of refs: first insert wins across the collect only while base > every owner.
    if (h[0] < m) {
        cdc::set_error("chunk store collect: fewer references than surviving containers");
        return CDC_EDEVICE;
    }

    // 2. Every allocation the call needs (the bounce buffer follows the plan,
    // still before anything is written).
    uint64_t *key_in = nullptr, *key = nullptr, *newloc = nullptr, *nblock = nullptr, *tstart = nullptr,
             *trel = nullptr, *gtiles = nullptr;
    uint32_t *slot_in = nullptr, *slot = nullptr, *new_slot = nullptr, *pending = nullptr, *map = d_map;
    uint8_t *dig = nullptr, *sort_tmp = nullptr, *bounce = nullptr;
    cdc_chunk_t *recs = nullptr;
    cdc::RetainGroup *groups = nullptr;
    cdc::StorePiece *pieces = nullptr;
    size_t sort_bytes = 0;
    unsigned end_bit = 1;
    while (end_bit < 64 && (st->arena_capacity >> end_bit)) ++end_bit;
    ST_ALLOC(mem.alloc(&key_in, m));
    ST_ALLOC(mem.alloc(&key, m));
    ST_ALLOC(mem.alloc(&slot_in, m));
    ST_ALLOC(mem.alloc(&slot, m));
    ST_ALLOC(mem.alloc(&newloc, m + 1));
    ST_ALLOC(mem.alloc(&nblock, cdc::store_scan_blocks(m) + 1));
    ST_ALLOC(mem.alloc(&dig, m * 32));
    ST_ALLOC(mem.alloc(&recs, m));
    ST_ALLOC(mem.alloc(&new_slot, m));
    ST_ALLOC(mem.alloc(&pending, cdc::kIndexPendingCap));
    ST_ALLOC(mem.alloc(&groups, m));
    ST_ALLOC(mem.alloc(&pieces, m));
    ST_ALLOC(mem.alloc(&tstart, m + 1));
    ST_ALLOC(mem.alloc(&trel, m));
    ST_ALLOC(mem.alloc(&gtiles, m));
    if (!map) ST_ALLOC(mem.alloc(&map, slots));  // the scatter writes one either way
    if (m) {
        ST_ALLOC(cdc::launch_retain_sort(nullptr, &sort_bytes, key_in, key, slot_in, slot, m, end_bit, s));
        ST_ALLOC(mem.alloc(&sort_tmp, sort_bytes));
    }
    NewTable nt;
    nt.t.slots = slots;
    ST_ALLOC(hipMalloc(&nt.t.tag, slots * 8));
    ST_ALLOC(hipMalloc(&nt.t.digest, slots * 32));
    ST_ALLOC(hipMalloc(&nt.t.owner, slots * 8));
    ST_ALLOC(hipMalloc(&nt.t.length, slots * 8));
    ST_ALLOC(hipMalloc(&nt.loc, slots * 8));
    lap(1);

    // 3. The survivors in arena order, their new offsets, the move groups.
    // groups, direct, bounced, bytes moved, overflow, W, new offset of the first moved byte, arena bytes afterwards
    uint64_t plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<cdc::RetainGroup> h_groups;
    if (m) {
        ST_TRY(cdc::launch_retain_list(st->t, st->loc, d_refs, val, key_in, slot_in, s));
        ST_TRY(cdc::launch_retain_sort(sort_tmp, &sort_bytes, key_in, key, slot_in, slot, m, end_bit, s));
        ST_TRY(cdc::launch_retain_layout(st->t, slot, m, newloc, nblock, dig, recs, s));
        ST_TRY(cdc::launch_retain_plan(key, newloc, m, retain_bounce_request(), h[3], groups, m, acc + 16, s));
        ST_TRY(hipMemcpyAsync(plan, acc + 16, sizeof plan, hipMemcpyDeviceToHost, s));
        ST_TRY(hipStreamSynchronize(s));
        if (plan[4]) {
            cdc::set_error("chunk store collect: the move plan did not close");
            return CDC_EDEVICE;
        }
        h_groups.resize(plan[0]);
        if (plan[0]) {
            ST_TRY(hipMemcpyAsync(h_groups.data(), groups, plan[0] * sizeof(cdc::RetainGroup), hipMemcpyDeviceToHost, s));
            ST_TRY(hipStreamSynchronize(s));
        }
        lap(2);
        if (plan[2]) ST_ALLOC(mem.alloc(&bounce, plan[5]));
        lap(1);
    }

    // 4. The new table, beside the live one: a failure here is still a refusal.
    ST_TRY(hipMemsetAsync(nt.t.tag, 0, slots * 8, s));
    ST_TRY(hipMemsetAsync(nt.t.owner, 0xFF, slots * 8, s));
    ST_TRY(hipMemsetAsync(map, 0xFF, slots * 4, s));
    uint64_t ins[5] = {0, 0, 0, 0, 0};  // the insert's counters, on scratch: the totals come from the contract
    if (m) {
        ST_TRY(cdc::launch_index_insert(nt.t, dig, recs, m, 0, new_slot, pending, nullptr, acc + 8, s));
        ST_TRY(cdc::launch_retain_scatter(slot, new_slot, newloc, m, nt.loc, map, s));
        ST_TRY(hipMemcpyAsync(ins, acc + 8, sizeof ins, hipMemcpyDeviceToHost, s));
        ST_TRY(hipStreamSynchronize(s));
        // A subset of what the table held cannot fill it; a pile of 64-bit key
        // collisions gathered over many puts could pass the one-batch cap.
        if (ins[0] != m || ins[3] || ins[4] > cdc::kIndexPendingCap) {
            cdc::set_error("chunk store collect: the survivors could not be inserted into the new table (" +
                           std::to_string(ins[0]) + " of " + std::to_string(m) + " placed, " +
                           std::to_string(ins[4]) + " 64-bit key collisions)");
            return CDC_ENOMEM;
        }
    }
    lap(3);

    // 5. The move: from here on the arena changes.  Groups run in stream order.
    if (!h_groups.empty()) {
        ST_TRY(cdc::launch_retain_pieces(key, newloc, m, groups, h_groups.size(), st->arena, bounce, pieces, tstart,
                                         nblock, trel, gtiles, s));
        uint64_t at = plan[6];  // new offset of the group's first byte
        for (size_t g = 0; g < h_groups.size(); ++g) {
            const cdc::RetainGroup &gr = h_groups[g];
            const uint64_t n = gr.b - gr.a;
            ST_TRY(cdc::launch_store_copy(pieces + gr.a, trel + gr.a, n, gr.bytes / cdc::kStoreTile + n, gtiles + g, s));
            if (!gr.direct && gr.bytes)
                ST_TRY(hipMemcpyAsync(st->arena + at, bounce, gr.bytes, hipMemcpyDeviceToDevice, s));
            at += gr.bytes;
        }
        ST_TRY(hipStreamSynchronize(s));
    }
    lap(4);

    // 6. Adopt the new table.
    const uint64_t new_used = plan[7];
    std::swap(st->t.tag, nt.t.tag);
    std::swap(st->t.digest, nt.t.digest);
    std::swap(st->t.owner, nt.t.owner);
    std::swap(st->t.length, nt.t.length);
    std::swap(st->loc, nt.loc);
    cdc_collect_stats_t r{};
    r.containers_before = st->st.unique_chunks;
    r.containers_after = m;
    r.arena_used_before = st->arena_used;
    r.arena_used_after = new_used;
    r.bytes_moved = plan[3];
    r.groups_direct = plan[1];
    r.groups_bounced = plan[2];
    st->st.chunks_written = h[0];
    st->st.bytes_written = h[1];
    st->st.unique_chunks = m;
    st->st.unique_bytes = h[2];
    st->arena_used = new_used;
    ++st->epoch;
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *out = r;
    std::memcpy(cdc::collect_split(), split, sizeof split);
    return CDC_OK;
}

}  // namespace

namespace cdc {

double *collect_split() {
    static thread_local double split[6];
    return split;
}

int store_retain(cdc_store *st, const unsigned long long *d_refs, uint32_t *d_map, cdc_collect_stats_t *out,
                 hipStream_t s) {
    return retain(st, d_refs, d_map, out, s);
}

bool store_scrub_view(const cdc_store *st, ScrubView *view, bool *stale) {
    if (!st->target || !st->target_containers) return false;
    *view = scrub_view(st);
    *stale = target_stale(st);
    return true;
}

StoreView store_view(const cdc_store *st) {
    return StoreView{st->device, st->stream, st->epoch, st->t.slots, st->t.length, st->loc, st->arena, st->d_slot};
}

IndexTable store_index(const cdc_store *st) { return st->t; }

void store_count_written(cdc_store *st, uint64_t chunks, uint64_t bytes) {
    st->st.chunks_written += chunks;
    st->st.bytes_written += bytes;
}

int64_t store_put_slots(cdc_store *st, const uint8_t *d_data, uint64_t data_len, const cdc_chunk_t *d_chunks,
                        const uint8_t *d_digests, uint64_t n, void *hip_stream) {
    const uint64_t lens[1] = {data_len}, first[2] = {0, n};
    const uint8_t *streams[1] = {d_data};
    return put(st, 1, streams, lens, first, d_chunks, d_digests, nullptr, hip_stream);
}

int64_t store_put_batch_slots(cdc_store *st, size_t n_streams, const uint8_t *const *d_streams, const uint64_t *lens,
                              const uint64_t *first, const cdc_chunk_t *d_chunks, const uint8_t *d_digests,
                              void *hip_stream) {
    return put(st, n_streams, d_streams, lens, first, d_chunks, d_digests, nullptr, hip_stream);
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

int cdc_store_set_hash(cdc_store_t *st, int hash) {
    const char *why = hash != CDC_HASH_SHA256 && hash != CDC_HASH_BLAKE2SP ? "unknown hasher (CDC_HASH_SHA256 or CDC_HASH_BLAKE2SP)"
                      : !st                                                  ? "NULL store"
                      : st->st.unique_chunks                                 ? "the store holds chunks (cdc_store_clear it first)"
                      : st->target                                           ? "a target store is attached"
                      : st->is_target                                        ? "the store is another store's target"
                                                                             : nullptr;
    if (why) {
        cdc::set_error(std::string("cdc_store_set_hash: ") + why);
        return CDC_EINVAL;
    }
    st->hash = hash;
    return CDC_OK;
}

int cdc_store_hash(const cdc_store_t *st) { return st ? st->hash : CDC_HASH_SHA256; }

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
    if (st->target_containers) return get_expanded(st, d_digests, n, d_out, out_cap, d_spans, s);
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

int64_t cdc_store_retain_device(cdc_store_t *st, const uint8_t *d_digests, size_t n, void *hip_stream) {
    if (!st) {
        cdc::set_error("NULL store");
        return CDC_EINVAL;
    }
    if (n && !d_digests) {
        cdc::set_error("cdc_store_retain_device: NULL argument");
        return CDC_EINVAL;
    }
    if (st->target_containers) {
        cdc::set_error("chunk store collect: the store holds target-kind containers (scrubbed); not supported");
        return CDC_ENOTSUP;
    }
    ST_TRY(hipSetDevice(st->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : st->stream;
    cdc::DeviceScratch mem;
    unsigned long long *refs = nullptr, *res = nullptr;
    ST_ALLOC(mem.alloc(&refs, st->t.slots));
    ST_ALLOC(mem.alloc(&res, 1));
    ST_TRY(hipMemsetAsync(refs, 0, st->t.slots * 8, s));
    ST_TRY(hipMemsetAsync(res, 0, 8, s));
    ST_TRY(cdc::launch_retain_refs(st->t, d_digests, n, refs, res, s));
    uint64_t missing = 0;
    ST_TRY(hipMemcpyAsync(&missing, res, 8, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    if (missing) {
        cdc::set_error("chunk store retain: " + std::to_string(missing) + " digest(s) not found");
        return CDC_ENOTFOUND;
    }
    cdc_collect_stats_t r{};
    const int rc = retain(st, refs, nullptr, &r, s);
    return rc ? rc : (int64_t)r.containers_after;
}

int cdc_debug_collect_split(double *ms, size_t n) {
    if (n && !ms) {
        cdc::set_error("cdc_debug_collect_split: NULL argument");
        return CDC_EINVAL;
    }
    if (n) std::memcpy(ms, cdc::collect_split(), (n < 6 ? n : 6) * sizeof(double));
    return 6;
}

int cdc_store_set_target(cdc_store_t *base, cdc_store_t *target) { return set_target(base, target); }

int cdc_store_scrub(cdc_store_t *base, int scrubber, cdc_handle_t *chunker, cdc_scrub_measurements_t *out,
                    void *hip_stream) {
    return scrub(base, scrubber, chunker, out, hip_stream);
}

int cdc_store_scrub_stats(const cdc_store_t *st, cdc_scrub_stats_t *out) {
    if (!st || !out) {
        cdc::set_error("NULL argument");
        return CDC_EINVAL;
    }
    out->cdc_bytes = st->st.unique_bytes - st->scrubbed_bytes;
    out->chunk_containers = st->st.unique_chunks - st->target_containers;
    out->target_containers = st->target_containers;
    out->keys = st->keys_used;
    out->target_bytes = st->target ? st->target->st.unique_bytes : 0;
    out->target_values = st->target ? st->target->st.unique_chunks : 0;
    return CDC_OK;
}

int64_t cdc_store_iterate_device(cdc_store_t *st, uint8_t *d_digests, uint8_t *d_kinds, uint64_t *d_lengths,
                                 uint64_t *d_key_first, size_t cap, void *hip_stream) {
    if (!st) {
        cdc::set_error("NULL store");
        return CDC_EINVAL;
    }
    if (cap && (!d_digests || !d_kinds || !d_lengths || !d_key_first)) {
        cdc::set_error("cdc_store_iterate_device: NULL destination");
        return CDC_EINVAL;
    }
    ST_TRY(hipSetDevice(st->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : st->stream;
    cdc::DeviceScratch mem;
    uint64_t *val = nullptr, n = 0;
    int rc = rank_slots(st, mem, -1, &val, &n, s);
    if (rc) return rc;
    if (n > cap || n == 0) return (int64_t)n;
    uint64_t *block = nullptr;
    ST_TRY(mem.alloc(&block, cdc::store_scan_blocks(n + 1) + 1));
    ST_TRY(hipMemsetAsync(d_key_first + n, 0, 8, s));
    ST_TRY(cdc::launch_store_iterate(st->t, scrub_view(st), val, d_digests, d_kinds, d_lengths, d_key_first, s));
    ST_TRY(cdc::launch_store_scan(d_key_first, n + 1, block, nullptr, s));
    ST_TRY(hipStreamSynchronize(s));
    return (int64_t)n;
}

int64_t cdc_store_size_distribution_device(cdc_store_t *st, uint64_t adjustment, uint64_t *d_sizes,
                                           uint32_t *d_counts, size_t cap, void *hip_stream) {
    if (!st) {
        cdc::set_error("NULL store");
        return CDC_EINVAL;
    }
    if (adjustment == 0) {
        cdc::set_error("cdc_store_size_distribution_device: adjustment must not be 0");
        return CDC_EINVAL;
    }
    if (cap && (!d_sizes || !d_counts)) {
        cdc::set_error("cdc_store_size_distribution_device: NULL destination");
        return CDC_EINVAL;
    }
    if (st->st.unique_chunks == 0) return 0;
    ST_TRY(hipSetDevice(st->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : st->stream;
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(st->d_acc) + 8;
    ST_TRY(hipMemsetAsync(acc, 0, 8, s));
    ST_TRY(cdc::launch_store_dist_max(st->t, acc, s));
    uint64_t max_len = 0;
    ST_TRY(hipMemcpyAsync(&max_len, acc, 8, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    const uint64_t n_bins = max_len / adjustment + 1;
    cdc::DeviceScratch mem;
    uint32_t *bins = nullptr;
    uint64_t *val = nullptr, *block = nullptr;
    hipError_t e = mem.alloc(&bins, n_bins);
    if (e == hipSuccess) e = mem.alloc(&val, n_bins);
    if (e == hipSuccess) e = mem.alloc(&block, cdc::store_scan_blocks(n_bins) + 1);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        cdc::set_error(std::string("chunk store size distribution: bins: ") + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? CDC_ENOMEM : CDC_EDEVICE;
    }
    ST_TRY(hipMemsetAsync(bins, 0, n_bins * 4, s));
    ST_TRY(cdc::launch_store_dist_bins(st->t, adjustment, bins, n_bins, val, block, acc + 1, s));
    uint64_t n = 0;
    ST_TRY(hipMemcpyAsync(&n, acc + 1, 8, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    if (n > cap || n == 0) return (int64_t)n;
    ST_TRY(cdc::launch_store_dist_emit(bins, n_bins, val, adjustment, d_sizes, d_counts, s));
    ST_TRY(hipStreamSynchronize(s));
    return (int64_t)n;
}

int64_t cdc_store_keys_device(cdc_store_t *st, uint8_t *d_keys, size_t cap, void *hip_stream) {
    if (!st) {
        cdc::set_error("NULL store");
        return CDC_EINVAL;
    }
    if (cap && !d_keys) {
        cdc::set_error("cdc_store_keys_device: NULL destination");
        return CDC_EINVAL;
    }
    if (!st->target_containers) return 0;
    if (target_stale(st)) {
        cdc::set_error("chunk store keys: the target store was cleared since these containers were scrubbed");
        return CDC_ENOTFOUND;
    }
    ST_TRY(hipSetDevice(st->device));
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : st->stream;
    cdc::DeviceScratch mem;
    uint64_t *val = nullptr, *block = nullptr;
    ST_TRY(mem.alloc(&val, st->t.slots));
    ST_TRY(mem.alloc(&block, cdc::store_scan_blocks(st->t.slots) + 1));
    const cdc::ScrubView v = scrub_view(st);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(st->d_acc) + 8;
    ST_TRY(cdc::launch_store_key_counts(st->t, v, val, s));
    ST_TRY(cdc::launch_store_scan(val, st->t.slots, block, acc, s));
    uint64_t n = 0;
    ST_TRY(hipMemcpyAsync(&n, acc, 8, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    if (n > cap || n == 0) return (int64_t)n;
    ST_TRY(cdc::launch_store_keys(st->t, v, val, d_keys, s));
    ST_TRY(hipStreamSynchronize(s));
    return (int64_t)n;
}

}  // extern "C"
