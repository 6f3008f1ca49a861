// engine.hpp -- device-side orchestration behind the C ABI.
//
// One Engine = one chunker handle bound to one GPU: a chunker object of
// reference src/chunkers/*.rs.  It validates the arguments of every call,
// dispatches device batches to its backend -- FastCDC's FastEngine
// (fast_engine.hpp), a segment-walk rule's (Rabin / Ultra / Leap / Seq / AE)
// WalkEngine (walk_engine.hpp), or the fixed-size path, which is one launch
// here -- keeps the result of a drain made on the caller's behalf, hands the
// hash calls (SHA-256, BLAKE2sp) to its HashEngine (hash_engine.hpp) and the
// calls on host memory to its HostPath (host_path.hpp).  Not thread-safe (the
// reference serialises through a Mutex, src/lib.rs:89-90).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "host_common.hpp"

namespace cdc {

class FastEngine;
class HashEngine;
class HostPath;
class WalkEngine;
struct WalkConfig;

class Engine {
  public:
    // Returns CDC_OK or a negative CDC_E* code (message via set_error()).
    static int create(cdc_algo_t algo, uint32_t min, uint32_t avg, uint32_t max,
                      int device, Engine **out);
    // SeqChunker::new(mode, sizes, config) (seq.rs:16-24): seq = {mode,
    // seq_length, jump_trigger, jump_size} (mode 0 increasing, 1 decreasing).
    static int create_seq(const uint32_t seq[4], uint32_t min, uint32_t avg, uint32_t max,
                          int device, Engine **out);
    // AE (DESIGN.md "AE"): mode 0 = Max, 1 = Min; window 0 = the default
    // (cdc_ae_default_window).
    static int create_ae(uint32_t mode, uint32_t window, uint32_t min, uint32_t avg, uint32_t max, int device,
                         Engine **out);
    ~Engine();

    // The host boundary: cdc_chunk_data, cdc_chunk_and_hash, cdc_fs_write,
    // cdc_write_* and the host-path debug entries are HostPath's.
    HostPath &host() { return *host_; }
    // SHA-256 of chunks of one device-resident stream (Sha256Hasher::hash).
    int sha256_device(const uint8_t *d_data, const cdc_chunk_t *d_chunks, size_t n,
                      uint8_t *d_digests, hipStream_t s);
    // The same over n streams in one launch, with either hasher (CDC_HASH_*:
    // cdc_hash_batch_device, cdc_sha256_batch_device); `who` names the entry
    // point in the refusals.
    int hash_batch(int hash, size_t n, const uint8_t *const *d_streams, const uint64_t *first,
                   const cdc_chunk_t *d_chunks, uint8_t *d_digests, hipStream_t s,
                   const char *who = "cdc_sha256_batch_device");
    int64_t chunk_batch_device(size_t n, const uint8_t *const *d_streams,
                               const uint64_t *lens, cdc_chunk_t *d_out,
                               size_t out_cap, uint64_t *first, hipStream_t stream);
    // The same, enqueued (cdc_chunk_batch_device_async): batches of more than
    // 8 MiB return before they complete, first[] filled by batch_sync() --
    // FastCDC's go back to back on the stream with no host wait, a walk rule's
    // to the WalkEngine's contexts.  Fixed-size batches run synchronously.
    int64_t chunk_batch_device_async(size_t n, const uint8_t *const *d_streams, const uint64_t *lens,
                                     cdc_chunk_t *d_out, size_t out_cap, uint64_t *first, hipStream_t stream);
    // Waits for every enqueued batch (resolving the last one); the total chunk
    // count of the last batch, or a negative code.
    int64_t batch_sync();
    size_t estimate(size_t len) const;
    // Strict bound: every FastCDC chunk but the last is >= 2*(min/2) bytes
    // (cut_gear starts testing at index 2*(min/2)).
    size_t min_chunk() const { return algo_ == CDC_ALGO_FASTCDC ? (min_ / 2) * 2 : min_; }
    size_t max_chunks(size_t len) const { return len / min_chunk() + 1; }
    // The longest chunk the rule cuts (FSChunker: the chunk size).
    size_t max_chunk() const { return algo_ == CDC_ALGO_FIXED ? min_ : max_; }
    size_t batch_max_chunks(size_t n, const uint64_t *lens) const;
    int set_gear(const uint64_t *gear);
    int set_rabin_poly(uint64_t poly);
    const char *describe() const { return describe_.c_str(); }
    // Kernel durations of the last batch (the backend's, read on request),
    // with hash_ms of the last hash call (either hasher).
    const cdc_timing_t &timing();
    // Kernel times of the FastCDC batch `back` calls before the last one
    // (event ring, include/chunkfs_amd_debug.h).
    int timing_back(uint32_t back, cdc_timing_t &out);
    cdc_algo_t algo() const { return algo_; }
    int device() const { return device_; }
    int fill_splitmix64(uint8_t *d_buf, size_t len, uint64_t seed, hipStream_t s);
    int read_bw(const uint8_t *d_buf, size_t len, int reps, double *ms);
    // Debug (include/chunkfs_amd_debug.h): FastEngine::debug_copy /
    // record_cap of a FastCDC handle.
    int64_t debug_copy(int what, void *out, size_t max_bytes);
    uint32_t record_cap() const;
    // What the walk engine derived and how its last synchronous batch ended
    // (WalkEngine::debug_params); -1 for a handle that is not a walk handle.
    int walk_params(uint64_t *v, size_t n) const;

  private:
    Engine() = default;
    // cfg: what a walk rule takes beyond the sizes (the defaults for cdc_create).
    static int create_handle(cdc_algo_t algo, WalkConfig &cfg, uint32_t min, uint32_t avg, uint32_t max, int device,
                             Engine **out);
    int init();
    friend class HostPath;  // (what it uses: host_path.hpp)
    // skip_small: the small kernel already declined these bytes (HostPath::chunk_host).
    int64_t batch_device(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                         size_t out_cap, uint64_t *first, hipStream_t stream, bool async, bool skip_small = false);
    // "A batch is in flight", whichever backend took it.  drain() completes
    // them (FastEngine::drain / WalkEngine::drain: the last batch's chunk
    // count or the first failure).
    bool in_flight() const;
    int64_t drain();
    // A drain made for another call: hold() keeps its result for batch_sync.
    int64_t drain_implicit();
    void hold(int64_t result);
    void report(const cdc_timing_t &batch);  // timing_ = the batch's, hash_ms kept
    int ensure_fixed(size_t n);
    int64_t run_fixed(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, uint64_t bytes,
                      cdc_chunk_t *d_out, uint64_t *first, hipStream_t s);
    // The backend of a FastCDC handle, of a Rabin / Ultra / Leap / Seq / AE
    // handle; a fixed-size handle has neither.
    std::unique_ptr<FastEngine> fast_;
    std::unique_ptr<WalkEngine> walk_;
    std::unique_ptr<HashEngine> hash_;  // every handle's: the hashers' scratch and launch
    std::unique_ptr<HostPath> host_;    // every handle's: the host boundary, allocated on first use

    cdc_algo_t algo_ = CDC_ALGO_FASTCDC;
    uint32_t min_ = 0, avg_ = 0, max_ = 0;
    int device_ = 0;
    int num_cus_ = 256;
    std::string describe_;

    hipStream_t own_stream_ = nullptr;
    hipEvent_t ev_[2] = {nullptr, nullptr};  // start, end: of a fixed-size batch, of read_bw's timed launches
    int64_t held_ = 0;              // result of the last implicit drain (hold)
    bool held_valid_ = false;
    // What cdc_last_timing reports: the backend's timing (the fixed-size
    // path's own) with hash_ms carried from the last hash call.
    cdc_timing_t timing_{};

    // Fixed-size path: one call's stream tables ++ first[n+1], staged in a
    // pinned, coherent block and mirrored in a device block (both grow-only;
    // gen counts the device block's allocations for CallTables::publish).
    struct Fixed {
        CallTables tab;
        void *h_block = nullptr, *d_block = nullptr;
        uint64_t *h_first = nullptr, *d_first = nullptr;  // [n+1]
        size_t streams = 0;
        uint64_t gen = 0;
    } fixed_;

    // Where pinned host memory and the copy helpers go: probed once, on first
    // use, for every backend and the host path.
    HostPlacement place_;
    bool place_probed_ = false;
    const HostPlacement &placement();
};

}  // namespace cdc
