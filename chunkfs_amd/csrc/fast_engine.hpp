// fast_engine.hpp -- the host side of the FastCDC kernels: the scan + resolve
// pipeline (fastcdc.hip) and the one-launch small kernel (small.hip).
//
// One FastEngine = one size triple with its masks, span geometry, device
// workspace and pinned staging: the handle's (Engine::fast_).  It runs
// synchronous batches to completion and keeps up to three async batches in
// flight, their resolves on a second stream.  Not thread-safe.
#pragma once
#include <memory>

#include "fastcdc.hpp"
#include "host_common.hpp"
#include "small.hpp"

namespace cdc {

class FastEngine {
  public:
    // The size checks of a FastCDC handle and its Debug string; no HIP call.
    // CDC_OK or CDC_EINVAL (message via set_error()).
    static int validate(uint32_t min, uint32_t avg, uint32_t max, std::string &describe);
    // Validated sizes on `device` (the current one, `num_cus` compute units):
    // masks, span size, record cap, the small kernel's budgets and every
    // CHUNKFS_AMD_* switch of the pipeline are settled here.
    static int create(uint32_t min, uint32_t avg, uint32_t max, int device, int num_cus,
                      std::unique_ptr<FastEngine> &out);
    ~FastEngine();

    // A call that has to complete the batches in flight first (another stream
    // or stream mode, a zero-copy batch, a regrown buffer, any batch that is
    // not pipelined) does so through drain() and reports that drain's result
    // in `drained`, which the handle holds for cdc_batch_sync; kNoDrain
    // otherwise.  A failed drain is also the call's return value.
    static constexpr int64_t kNoDrain = INT64_MIN;
    // One batch, complete at return: first[n+1] and the chunks in d_out.
    // Arguments as validated by Engine::batch_device; `place`: the handle's
    // placement, through which the pinned staging is allocated.  A single
    // stream the small kernel can take goes to it first (skip_small: it
    // already declined these bytes).  Returns the chunk count or a negative
    // code; timing() then describes the batch.
    int64_t chunk_batch(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                        size_t out_cap, uint64_t *first, hipStream_t s, const HostPlacement &place, bool skip_small,
                        int64_t &drained);
    // Async batches: scan + resolve enqueued with no host wait (by default the
    // resolve on a second stream, beside the next batch's scan); first[] is
    // filled when the batch is collected, by the submit three later or by
    // drain().  Returns 0 or a negative code.
    bool takes_async(size_t n, uint64_t bytes) const { return n > 0 && bytes > kSmallBatch; }
    int64_t submit(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                   size_t out_cap, uint64_t *first, hipStream_t s, const HostPlacement &place, int64_t &drained);
    bool in_flight() const { return any_; }
    // Every batch in flight collected in order: the last one's chunk count,
    // or the first failure.
    int64_t drain();

    // Nothing in flight (Engine::set_gear drains first).
    int set_gear(const uint64_t *gear);

    // Kernel durations of the last batch: a batch whose done word was seen
    // returns before its kernels retire, and its events are read here, on
    // first request.  timing_back: the batch `back` calls before the last one
    // (event ring, include/chunkfs_amd_debug.h).  Nothing in flight.
    const cdc_timing_t &timing();
    int timing_back(uint32_t back, cdc_timing_t &out);
    // Debug (include/chunkfs_amd_debug.h): an intermediate array of the last
    // pipeline batch.  what: 0 = per-span candidate counts (u32), 1 =
    // candidate records (u32, record_cap() per span).  2..4: the scratch of
    // the last call when the one-launch kernel took it (small.hip): per-block
    // record counts, per-block record regions, the device copy of a host
    // input; 5..7: the same arrays whole, with what earlier calls left beyond
    // the last one's blocks.  Returns bytes copied.
    int64_t debug_copy(int what, void *out, size_t max_bytes);
    uint32_t record_cap() const { return cap_; }

    // One small stream in one launch (small.hip), for chunk_batch and the
    // host path: CDC_OK, kSmallFallback (a budget was exceeded: run the
    // regular pipeline) or a CDC_E* code.
    static constexpr int kSmallFallback = 1;
    bool small_ok(uint64_t len) const;
    // The host path gives the kernel its input in the pinned ring slot itself
    // (no H2D copy) unless CHUNKFS_AMD_SMALL_ZC=0, and streams it
    // (CHUNKFS_AMD_SMALL_FEED): 1 = launch first, then the copy with feed
    // words; 0 = the whole copy, then the launch; 2 = the feed copy, then the
    // launch (A/B).
    bool small_zero_copy() const { return small_zc_; }
    int small_feed() const { return small_feed_; }
    // Streamed host input: the kernel is launched first, then the bytes are
    // copied from src into dst (the ring slot that `data` addresses) piece by
    // piece, each piece announced by a feed word (ready / its device address
    // ready_dev: the slot's kFeedPieces words).
    struct SmallFeed {
        const uint8_t *src;
        uint8_t *dst;
        volatile uint64_t *ready;
        const uint64_t *ready_dev;
        CopyPool *pool;
    };
    int run_small(const uint8_t *data, uint64_t len, cdc_chunk_t *d_out, size_t out_cap, uint64_t *first,
                  hipStream_t s, const HostPlacement &place, bool host_input = false,
                  const SmallFeed *feed = nullptr);
    uint64_t small_calls() const { return small_calls_; }
    uint64_t small_fallbacks() const { return small_fallbacks_; }
    double small_copy_s() const { return small_copy_s_; }  // the last streamed call's host copy time

  private:
    FastEngine() = default;
    int ensure_workspace(uint64_t spans, size_t n);
    int ensure_host_staging(size_t n, const HostPlacement &place);
    // One batch enqueued (scan + resolve); two_stream: the resolve on res_stream_.
    int64_t enqueue(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                    size_t out_cap, uint64_t *first, uint64_t bytes, hipStream_t s, const HostPlacement &place,
                    bool timed, bool two_stream, int64_t &drained);
    int collect(int rec);

    int device_ = 0;
    int num_cus_ = 256;
    FastParams fp_{};
    uint32_t span_log2_ = 16;
    uint32_t small_span_log2_ = 16;  // spans of batches <= kSmallBatch bytes
    uint32_t cap_ = 0, smax_ = 0;
    uint64_t *d_gear_ = nullptr;

    // Workspace arena (grow-only).
    void *ws_ = nullptr;
    uint64_t ws_spans_ = 0, ws_gen_ = 0;  // generation: uploaded stream tables are valid within one
    size_t ws_streams_ = 0;
    p3::Chains ch3_{};    // chunk starts spilled past the resolve's LDS
    p3::Resolve rs3_{};   // look-back descriptors (generation-tagged, never re-zeroed)
    uint64_t res_gen_ = 0;
    // Batches in flight: device tables and candidates in four slots (slot =
    // sequence number % 4) whose uploaded tables are kept to skip unchanged
    // H2D copies; host staging in three blocks (batch record k % 3, below):
    // batch k's block -- tables going in, stats ++ first[] coming back -- is
    // read at its collection, before submit k+3 reuses it.  A device slot
    // outlives its host block, so when batch k is submitted the slot's
    // previous user k-4 is complete (k-3 was collected): no stream wait guards
    // it, even with the resolves on a second stream.
    static constexpr int kSlots = 4, kHostSlots = 3;
    struct FastSlot {
        Candidates cand{};
        const uint8_t **d_ptrs = nullptr;
        uint64_t *d_lens = nullptr, *d_sb = nullptr, *d_tails = nullptr, *stats = nullptr;
        std::vector<uint64_t> tables;    // ptrs ++ lens as last uploaded (skip the H2D when unchanged)
        uint64_t tables_gen = ~0ull;
        uint32_t n_tails = 0;            // ragged last spans of those tables
    } fs_[kSlots];
    // Pinned, device-visible (coherent) host staging, one block per batch
    // record: the small per-call tables going in, stats ++ first[n+1] coming
    // back (written by the resolve kernel directly, no copy).  The small
    // kernel reports into block 0's stats ++ first[].
    struct HostBlock {
        uint64_t *ptrs = nullptr, *lens = nullptr, *sb = nullptr, *tails = nullptr;  // [W] [W] [W] [W]
        uint64_t *stats = nullptr, *first = nullptr;                                  // [kStatWords] [n+1]
    } hb_[kHostSlots];
    void *h_stage_ = nullptr;
    size_t h_stage_streams_ = 0;
    // Batch records, by sequence number % 3: live from its launches to its
    // collection; the last one also tells debug_copy its slot and spans.
    struct FastBatch {
        bool live = false, timed = true, two_stream = false;
        int slot = 0;                // device slot
        size_t n = 0;
        uint64_t *first = nullptr;  // the caller's first[n+1]
        uint64_t seq = 0, bytes = 0, spans = 0;
    } fb_[kHostSlots];
    uint64_t seq_ = 0;              // batches submitted
    hipStream_t stream_ = nullptr;  // the stream of the batches in flight
    bool any_ = false;              // a batch is in flight
    bool any_two_stream_ = false;   // ... with their resolves on res_stream_
    // Async batches on two streams (default, CHUNKFS_AMD_OVERLAP=1): batch k's
    // resolve on res_stream_ behind scan_ev_[slot k], batch k+1's scan on the
    // caller's stream right behind scan k.  A resolve block (148 KiB of LDS)
    // and a scan block (136 KiB) never share a CU, so nothing co-resides: the
    // next scan's blocks take each CU as its resolve block retires -- the
    // kernel-to-kernel gaps and the resolve's ragged end leave the step
    // (0.2557 vs 0.2744 ms sustained, profiles/r06/r06p_*).  res_ev_ orders the
    // caller's stream after the resolves at a drain.  CHUNKFS_AMD_OVERLAP=0:
    // one stream.  (A second kernel set sized to co-reside measured slower,
    // 0.33 vs 0.278 ms per step, profiles/r06/r06a_*, and was removed.)
    bool two_stream_on_ = true;
    hipStream_t res_stream_ = nullptr;
    hipEvent_t scan_ev_[kSlots] = {};
    hipEvent_t res_ev_ = nullptr;
    hipEvent_t res_done_[kHostSlots] = {};  // untimed batch k's resolve end on res_stream_ (record k % 3)

    // Events (start, scan end, resolve end) in a ring of kTimeRing slots,
    // batch k in slot k % kTimeRing.  Async batches record them 1 in
    // event_every_ (CHUNKFS_AMD_EVENT_EVERY): each event costs the stream
    // ~4 us.
    static constexpr uint32_t kTimeRing = 64;
    hipEvent_t tev_[kTimeRing][3] = {};
    bool tev_timed_[kTimeRing] = {};  // events recorded for ring slot
    int event_every_ = 4;
    cdc_timing_t timing_{};
    bool timing_pending_ = false;     // events not read yet (see timing())
    uint64_t timing_seq_ = 0;         // the batch timing_ describes

    // Small kernel: on for sparse masks unless CHUNKFS_AMD_SMALL=0.
    bool small_on_ = false, small_zc_ = true;
    int small_feed_ = 1;
    bool small_feed_pool_ = true;  // the feed copy on the copy pool (CHUNKFS_AMD_SMALL_FEED_POOL=0: caller only, A/B)
    uint32_t small_pmin_ = 0;      // min(popcount mask_s, popcount mask_l): records ~ 2^-pmin per byte
    void *small_mem_ = nullptr;
    small::Scratch small_ws_{};
    uint64_t small_calls_ = 0, small_fallbacks_ = 0;
    uint64_t small_seq_ = 0;       // launch sequence number (feed words, block publication tags)
    double small_copy_s_ = 0;
    // The last FastCDC call, when the small kernel took it (debug_copy): its
    // length (0: a pipeline batch, a fallback or none), whether its input was
    // host memory (device copy written) and its stream.
    uint64_t small_last_len_ = 0;
    bool small_last_staged_ = false;
    hipStream_t small_last_stream_ = nullptr;
};

}  // namespace cdc
