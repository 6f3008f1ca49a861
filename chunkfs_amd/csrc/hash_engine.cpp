// hash_engine.cpp -- the chunk hashers' scratch buffers and their launch.
#include "hash_engine.hpp"

#include <cstring>

#include "blake2sp.hpp"
#include "sha256.hpp"

namespace cdc {

int HashEngine::create(int num_cus, std::unique_ptr<HashEngine> &out) {
    std::unique_ptr<HashEngine> e(new HashEngine());
    e->num_cus_ = num_cus;
    for (auto &ev : e->ev_) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipMalloc(&e->d_counter_, (1 + kShaBuckets) * sizeof(unsigned long long)));
    out = std::move(e);
    return CDC_OK;
}

HashEngine::~HashEngine() {
    (void)hipFree(d_tab_);
    (void)hipHostFree(h_tab_);
    (void)hipFree(d_order_);
    (void)hipFree(d_counter_);
    for (auto &ev : ev_)
        if (ev) (void)hipEventDestroy(ev);
}

int HashEngine::run(int hash, size_t n, const uint8_t *const *d_streams, const uint64_t *first,
                    const cdc_chunk_t *d_chunks, uint8_t *d_digests, uint64_t total, hipStream_t stream, float *ms) {
    const size_t words = 2 * n + 1;
    if (tab_cap_ < words) {
        (void)hipFree(d_tab_);
        (void)hipHostFree(h_tab_);
        d_tab_ = h_tab_ = nullptr;
        tab_cap_ = 0;
        const size_t want = words + 64;
        HIP_TRY(hipMalloc(&d_tab_, want * 8));
        HIP_TRY(hipHostMalloc(&h_tab_, want * 8, hipHostMallocDefault));
        tab_cap_ = want;
    }
    if (order_cap_ < total) {
        (void)hipFree(d_order_);
        d_order_ = nullptr;
        order_cap_ = 0;
        const uint64_t want = total + total / 8 + 1024;
        HIP_TRY(hipMalloc(&d_order_, want * sizeof(uint32_t)));
        order_cap_ = want;
    }
    std::memcpy(h_tab_, first, (n + 1) * 8);
    for (size_t i = 0; i < n; ++i) h_tab_[n + 1 + i] = reinterpret_cast<uint64_t>(d_streams[i]);
    HIP_TRY(hipMemcpyAsync(d_tab_, h_tab_, words * 8, hipMemcpyHostToDevice, stream));
    ShaBatch b{};
    b.chunks = reinterpret_cast<const cdc_chunk_pod *>(d_chunks);
    b.n_chunks = total;
    b.first = d_tab_;
    b.base = d_tab_ + n + 1;
    b.n_streams = (uint32_t)n;
    b.digests = reinterpret_cast<uint32_t *>(d_digests);
    b.counter = d_counter_;
    b.order = d_order_;
    HIP_TRY(hipEventRecord(ev_[0], stream));
    HIP_TRY(hash == CDC_HASH_BLAKE2SP ? launch_blake2sp(b, num_cus_, stream) : launch_sha256(b, num_cus_, stream));
    HIP_TRY(hipEventRecord(ev_[1], stream));
    HIP_TRY(hipStreamSynchronize(stream));  // (also: the pinned table may be rewritten by the next call)
    HIP_TRY(hipEventElapsedTime(ms, ev_[0], ev_[1]));
    return CDC_OK;
}

}  // namespace cdc
