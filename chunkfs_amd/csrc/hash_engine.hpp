// hash_engine.hpp -- the host side of the chunk hashers (sha256.hip,
// blake2sp.hip): the device scratch a hash launch needs and the launch itself.
//
// One HashEngine = the handle's (Engine::hash_), for either hasher.  Its
// buffers are grow-only and reused by every call; a call is complete at return.
// Not thread-safe.
#pragma once
#include <memory>

#include "host_common.hpp"

namespace cdc {

class HashEngine {
  public:
    // On the current device.
    static int create(int num_cus, std::unique_ptr<HashEngine> &out);
    ~HashEngine();

    // One launch over the `total` > 0 chunks of n streams, with hasher `hash`
    // (CDC_HASH_*); arguments as validated by Engine::hash_batch.  The stream
    // table (first[], bases) goes up through a pinned block with one H2D copy.
    // Complete at return; *ms: the order kernels and the hash kernel.
    int run(int hash, size_t n, const uint8_t *const *d_streams, const uint64_t *first, const cdc_chunk_t *d_chunks,
            uint8_t *d_digests, uint64_t total, hipStream_t stream, float *ms);

  private:
    HashEngine() = default;

    int num_cus_ = 256;
    unsigned long long *d_counter_ = nullptr;     // work counter ++ length histogram [1 + kShaBuckets]
    uint64_t *d_tab_ = nullptr, *h_tab_ = nullptr;  // the batch's stream table: first[n+1] ++ bases[n] (h_: pinned)
    size_t tab_cap_ = 0;                           // ... in words
    uint32_t *d_order_ = nullptr;                  // claim order (longest chunk first)
    uint64_t order_cap_ = 0;
    hipEvent_t ev_[2] = {nullptr, nullptr};        // before the order kernels, after the hash kernel
};

}  // namespace cdc
