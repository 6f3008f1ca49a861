// walk_engine.hpp -- the host side of the segment-walk engine (walk.hip):
// Rabin / UltraCDC / LeapCDC / SeqCDC / AE.
//
// One WalkEngine = one rule with its sizes, device tables, workspace and
// pinned host block: the handle's (Engine::walk_), which chunks synchronous
// batches itself and hands async ones to its contexts -- WalkEngines of the
// same configuration, each with a stream and a host worker thread.  Not
// thread-safe.
#pragma once
#include <memory>

#include "../../include/chunkfs_amd_cdc_params.h"
#include "host_common.hpp"
#include "walk.hpp"

namespace cdc {

// What a rule takes beyond the sizes.  SeqChunker::new(mode, sizes, config)
// (seq.rs:16-24): mode 0 increasing, 1 decreasing.  AE (DESIGN.md "AE"): mode
// 0 = Max, 1 = Min; window 0 = the default (cdc_ae_default_window), resolved
// by WalkEngine::validate.
struct WalkConfig {
    uint32_t seq_mode = 0, seq_length = CDC_SEQ_LENGTH, seq_jump_trigger = CDC_SEQ_JUMP_TRIGGER,
             seq_jump_size = CDC_SEQ_JUMP_SIZE;
    uint32_t ae_mode = CDC_AE_MODE_MAX, ae_window = 0;
};

class WalkEngine {
  public:
    // The size and rule checks of a walk handle and its Debug string; no HIP
    // call.  CDC_OK or CDC_EINVAL (message via set_error()).
    static int validate(cdc_algo_t algo, uint32_t min, uint32_t avg, uint32_t max, WalkConfig &cfg,
                        std::string &describe);
    // A validated configuration on `device` (the current one).
    static int create(cdc_algo_t algo, uint32_t min, uint32_t avg, uint32_t max, const WalkConfig &cfg, int device,
                      std::unique_ptr<WalkEngine> &out);
    ~WalkEngine();

    // One batch, complete at return: first[n+1] and the chunks in d_out.
    // Arguments as validated by Engine::batch_device; `place`: the handle's
    // placement, through which the pinned host block is allocated.  Returns
    // the chunk count or a negative code; timing() then describes the batch.
    int64_t chunk_batch(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                        size_t out_cap, uint64_t *first, hipStream_t s, const HostPlacement &place);
    const cdc_timing_t &timing() const { return timing_; }

    // Async batches: two contexts (CHUNKFS_AMD_WALK_CTX: 2..4) run alternate
    // batches synchronously, each on its own stream and host worker thread,
    // so one batch's walks and fix-up rounds overlap the next batch's bitmap
    // pass on the device (a walk call keeps host logic between its kernels:
    // the round loop).  A batch is ordered after the work already on `s` (the
    // caller's stream): an event recorded there, which the context's stream
    // waits for.  CHUNKFS_AMD_WALK_ASYNC=0: every batch completes in its call.
    bool takes_async(size_t n, uint64_t bytes) const { return async_ && n > 0 && bytes > kSmallBatch; }
    int64_t submit(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                   size_t out_cap, uint64_t *first, hipStream_t s, const HostPlacement &place);
    bool in_flight() const { return in_flight_; }
    // Every batch in flight completed: the last one's chunk count (timing()
    // is then its context's), or the first failure.
    int64_t drain();

    // Validated by Engine::set_rabin_poly, nothing in flight: new tables, the
    // workspace laid out again, the contexts made again at their next batch.
    int set_rabin_poly(uint64_t poly);

    // Debug (include/chunkfs_amd_debug.h cdc_debug_walk_params): what init()
    // derived, then the segment count of the last synchronous batch and how
    // it ended, into v[0..n).  Returns the values the engine has (kDebugWords).
    static constexpr int kDebugWords = 9;
    int debug_params(uint64_t *v, size_t n) const;

  private:
    WalkEngine() = default;
    int init();
    int load_tables(uint64_t rabin_poly);
    int ensure_host_block(size_t n, const HostPlacement &place);
    int ensure_workspace(uint64_t segs, size_t n);
    int run(const StreamTable &st, cdc_chunk_t *d_out, uint64_t out_cap, size_t n, uint64_t *first, hipStream_t s);

    cdc_algo_t algo_ = CDC_ALGO_RABIN;
    uint32_t min_ = 0, avg_ = 0, max_ = 0;
    WalkConfig cfg_;
    int device_ = 0;
    uint64_t rabin_poly_ = CDC_RABIN_POLY;

    walk::WalkParams wp_{};
    uint32_t seg_log2_ = 14;
    uint32_t max_rounds_ = 16;     // Jacobi fix-up rounds before the serial pass
    uint32_t ahead_after_ = 8;     // rounds of plain Jacobi before run-ahead re-walks
    uint32_t ahead_max_ = 64;      // segments one lane may re-walk in a run-ahead round
    bool fused_ = true;            // fused end kernel (CHUNKFS_AMD_WALK_FUSED=0: sum / prefix / first + copies, A/B)
    uint64_t *d_tabs_ = nullptr;   // [768] rabin mod/out + leap hash tables
    hipEvent_t ev_[3] = {nullptr, nullptr, nullptr};  // call start, walk end, output end

    // Workspace arena (grow-only), with the device stream tables.
    void *ws_ = nullptr;
    uint64_t ws_segs_ = 0, ws_gen_ = 0;
    size_t ws_streams_ = 0;
    walk::WalkState st_{};
    uint64_t *go_ = nullptr;       // finish_kernel's verdict word for the gated emit
    bool flags_clean_ = false;     // the flag blocks hold the init pattern (the last call's end kernel reset them)

    // Pinned, device-visible (coherent) host block: the call's stream tables
    // going in (read over PCIe by zero-copy batches); first[n+1] and flags[4]
    // ++ the fix-up round flag blocks coming back (written by finish_kernel
    // directly, or copied).
    void *h_block_ = nullptr;
    size_t h_streams_ = 0;
    uint64_t *h_first_ = nullptr, *h_flags_ = nullptr;
    CallTables tab_;

    cdc_timing_t timing_{};
    uint64_t last_segs_ = 0;   // debug_params: segments of the last synchronous batch
    uint32_t last_end_ = 0;    // ... and its end: 0 fused finish + gated emit, 1 gated emit, 2 ungated emit

    // Async contexts (submit / drain).
    struct Worker;
    static constexpr int kCtxMax = 4;
    std::unique_ptr<Worker> ctx_[kCtxMax];
    int n_ctx_ = 2;            // contexts in use (CHUNKFS_AMD_WALK_CTX, 2..4)
    bool async_ = true;        // CHUNKFS_AMD_WALK_ASYNC=0; false in a context
    bool in_flight_ = false;   // a batch was submitted since the last drain
    uint64_t seq_ = 0;         // batches submitted
};

}  // namespace cdc
