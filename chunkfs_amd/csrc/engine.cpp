// engine.cpp -- host orchestration of the gfx950 chunking pipeline.
//
// Per batch (DESIGN.md "Pipeline and kernels"):
//   H2D of three tiny per-stream tables (skipped when unchanged) -> scan ->
//   next (record links) -> walk (writes the chunks to HBM and first[n+1] + stats
//   straight into coherent pinned host memory) -> one stream sync.
// Everything runs on one HIP stream; candidates, chains and the output never
// leave HBM.
#include "engine.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/chunkfs_amd_tables.h"
#include "fastcdc.hpp"
#include "sha256.hpp"
#include "walk_engine.hpp"

namespace cdc {

namespace {
thread_local std::string g_last_error;

#ifndef CDC_MIN_SPAN_LOG2
#define CDC_MIN_SPAN_LOG2 16
#endif
constexpr uint32_t kMinSpanLog2 = CDC_MIN_SPAN_LOG2;  // 64 KiB spans at least (experiment builds may raise it)
constexpr uint32_t kMaxSpanLog2 = 17;  // ... and at most 128 KiB unless the max chunk needs more

// fastcdc 3.1.0 v2020 FastCDC::new asserts (VERIFY).
constexpr uint32_t kMinimumMin = 64, kMinimumMax = 1048576;
constexpr uint32_t kAverageMin = 256, kAverageMax = 4194304;
constexpr uint32_t kMaximumMin = 1024, kMaximumMax = 16777216;
}  // namespace

void set_error(const std::string &msg) { g_last_error = msg; }
const char *last_error() { return g_last_error.c_str(); }

int Engine::create(cdc_algo_t algo, uint32_t min, uint32_t avg, uint32_t max,
                   int device, Engine **out) {
    if (!out) {
        set_error("cdc_create: out is NULL");
        return CDC_EINVAL;
    }
    *out = nullptr;
    if (algo == CDC_ALGO_RABIN || algo == CDC_ALGO_ULTRA || algo == CDC_ALGO_LEAP || algo == CDC_ALGO_SEQ ||
        algo == CDC_ALGO_AE) {
        WalkConfig cfg;  // (the rule's defaults)
        return create_walk(algo, cfg, min, avg, max, device, out);
    }
    if (algo != CDC_ALGO_FASTCDC && algo != CDC_ALGO_FIXED) {
        set_error("SuperCDC is not implemented on MI355X: its chunk records (supercdc.rs:10, 37-50) "
                  "follow cdc-chunkers 0.1.3, absent offline (SURVEY.md §8c)");
        return CDC_ENOTSUP;
    }
    Engine *e = new Engine();
    e->algo_ = algo;
    e->min_ = min;
    e->avg_ = avg;
    e->max_ = max;
    e->device_ = device;
    if (algo == CDC_ALGO_FASTCDC) {
        if (min < kMinimumMin || min > kMinimumMax || avg < kAverageMin ||
            avg > kAverageMax || max < kMaximumMin || max > kMaximumMax) {
            set_error("FastCDC sizes out of range (fastcdc v2020 asserts: min 64..1MiB, "
                      "avg 256..4MiB, max 1KiB..16MiB)");
            delete e;
            return CDC_EINVAL;
        }
        // The rule has no defined answer below these orderings: with max < min
        // every chunk is max bytes, more than the len / min + 1 that the output
        // and the workspace are sized for; with max < avg the published first
        // loop runs to a centre past the clipped remainder.  (min > avg is
        // well defined: the first loop is empty.)
        if (max < min || max < avg) {
            set_error("FastCDC sizes out of order: max must be >= min and >= avg");
            delete e;
            return CDC_EINVAL;
        }
        const unsigned bits = (unsigned)std::lround(std::log2((double)avg));
        FastParams &fp = e->fp_;
        fp.min = min;
        fp.avg = avg;
        fp.max = max;
        fp.mask_s = CHUNKFS_AMD_MASKS[bits + 1];
        fp.mask_l = CHUNKFS_AMD_MASKS[bits - 1];
        fp.cmask = fp.mask_s & fp.mask_l;
        const uint64_t all = fp.mask_s | fp.mask_l;
        const uint32_t top = 63 - (uint32_t)__builtin_clzll(all);
        if (top > 47) {  // the 3-lane carry is exact mod 2^48 only
            set_error("mask tests bit >= 48: unsupported");
            delete e;
            return CDC_EINVAL;
        }
        fp.trunc = top;
        const uint32_t wlo = (uint32_t)__builtin_ctzll(all);
        fp.cm_align = (wlo <= 32 && (all >> wlo) <= 0xFFFFFFFFull) ? 1u : 0u;
        fp.tshift = fp.cm_align ? 32 - wlo : 0;
        fp.cm32 = (uint32_t)((fp.cmask << fp.tshift) >> 32);
        fp.cm_lo = (uint32_t)fp.cmask;
        fp.cm_hi = (uint32_t)(fp.cmask >> 32);
        fp.mask_s_sh = fp.mask_s << fp.tshift;
        fp.mask_l_sh = fp.mask_l << fp.tshift;
        if (const char *d = std::getenv("CHUNKFS_AMD_DIAG")) fp.diag = (uint32_t)std::atoi(d);
        if (const char *v = std::getenv("CHUNKFS_AMD_EVENT_EVERY")) e->event_every_ = std::max(1, std::atoi(v));
        if (const char *v = std::getenv("CHUNKFS_AMD_OVERLAP")) e->two_stream_on_ = std::atoi(v) != 0;  // (A/B; default on)
        uint32_t l2 = ceil_log2(max);
        e->span_log2_ = l2 > kMinSpanLog2 ? l2 : kMinSpanLog2;
        {
            // Up to 128 KiB spans while a resolve window (11 spans) expects <=
            // 384 records, half its budget (4/8/16 KiB: 352): half the scan's
            // per-span epilogues (scan 0.222 -> 0.203 ms per GiB) and half the
            // resolve blocks, which then leave half the CUs to the next
            // batch's scan on the two streams (0.262 -> 0.237 ms per step,
            // profiles/r06/r06zc_*).  (256 KiB: windows overflow to the slow
            // global path.)
            const uint32_t pcm = (uint32_t)__builtin_popcountll(fp.cmask);
            while (e->span_log2_ < kMaxSpanLog2 && 11 * ((2ull << e->span_log2_) >> (pcm < 63 ? pcm : 63)) <= 384)
                ++e->span_log2_;
        }
        if (const char *v = std::getenv("CHUNKFS_AMD_SPAN"))  // experiments: span log2 (>= the max's, >= 14)
            e->span_log2_ = (uint32_t)std::max<int>(std::atoi(v), (int)std::max(l2, 14u));
        e->small_span_log2_ = l2 > 14 ? l2 : 14;
        if (const char *v = std::getenv("CHUNKFS_AMD_SMALL_SPAN")) {  // experiments: 0 = off
            const int x = std::atoi(v);
            e->small_span_log2_ = x == 0 ? e->span_log2_ : (uint32_t)std::max<int>(x, (int)std::max(l2, 14u));
        }
        if (e->small_span_log2_ > e->span_log2_) e->small_span_log2_ = e->span_log2_;
        const uint64_t span = 1ull << e->span_log2_;
        const uint32_t pc = (uint32_t)__builtin_popcountll(fp.cmask);
        uint64_t cap = 8 * (span >> (pc < 63 ? pc : 63));
        if (cap < 64) cap = 64;
        if (cap > 256) cap = 256;
        e->cap_ = (uint32_t)cap;
        e->smax_ = (uint32_t)(span / ((min / 2) * 2) + 2);
        // Small-stream path (small.hip): its per-lane and per-block record
        // budgets assume sparse hits, ~2^-10 per position or rarer.
        const uint32_t pmin = (uint32_t)std::min(__builtin_popcountll(fp.mask_s), __builtin_popcountll(fp.mask_l));
        e->small_on_ = pmin >= 10;
        e->small_pmin_ = pmin;
        if (const char *v = std::getenv("CHUNKFS_AMD_SMALL")) e->small_on_ = e->small_on_ && std::atoi(v) != 0;
        if (const char *v = std::getenv("CHUNKFS_AMD_SMALL_ZC")) e->small_zc_ = std::atoi(v) != 0;
        if (const char *v = std::getenv("CHUNKFS_AMD_SMALL_FEED")) e->small_feed_ = std::atoi(v);
        if (const char *v = std::getenv("CHUNKFS_AMD_SMALL_FEED_POOL")) e->small_feed_pool_ = std::atoi(v) != 0;
        char buf[256];
        std::snprintf(buf, sizeof buf,
                      "FastCDC (2020), sizes: SizeParams { min: %u, avg: %u, max: %u } "
                      "[MI355X gfx950]",
                      min, avg, max);
        e->describe_ = buf;
    } else {
        if (min == 0) {
            set_error("FSChunker chunk size must be > 0");
            delete e;
            return CDC_EINVAL;
        }
        char buf[128];
        std::snprintf(buf, sizeof buf, "Fixed size chunking, chunk size: %u [MI355X gfx950]", min);
        e->describe_ = buf;
    }
    const int rc = e->init();
    if (rc != CDC_OK) {
        delete e;
        return rc;
    }
    *out = e;
    return CDC_OK;
}

int Engine::init() {
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device_ < 0 || device_ >= count) {
        set_error("device index out of range");
        return CDC_EDEVICE;
    }
    HIP_TRY(hipSetDevice(device_));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("chunkfs_amd kernels are built for gfx950 only; device is ") +
                  prop.gcnArchName);
        return CDC_EDEVICE;
    }
    num_cus_ = prop.multiProcessorCount;
    HIP_TRY(hipStreamCreateWithFlags(&own_stream_, hipStreamNonBlocking));
    for (auto &ev : ev_) HIP_TRY(hipEventCreate(&ev));
    if (algo_ == CDC_ALGO_FASTCDC)  // (no other handle records or reads the ring: timing_back refuses it)
        for (auto &slot : tev_)
            for (auto &ev : slot) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipMalloc(&d_gear_, 256 * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(&d_counter_, (1 + kShaBuckets) * sizeof(unsigned long long)));  // SHA-256 counter + histogram
    HIP_TRY(hipMemcpy(d_gear_, CHUNKFS_AMD_GEAR, 256 * sizeof(uint64_t), hipMemcpyHostToDevice));
    return CDC_OK;
}

Engine::~Engine() {
    if (device_ >= 0) (void)hipSetDevice(device_);
    if (in_flight()) (void)drain();
    walk_.reset();
    if (own_stream_) (void)hipStreamSynchronize(own_stream_);
    if (res_stream_) (void)hipStreamSynchronize(res_stream_);
    (void)hipFree(ws_);
    (void)hipFree(small_mem_);
    (void)hipFree(d_gear_);
    (void)hipFree(d_data_);
    (void)hipFree(d_out_);
    (void)hipFree(d_dig_);
    (void)hipFree(d_sha_tab_);
    (void)hipHostFree(h_sha_tab_);
    (void)hipFree(d_sha_order_);
    (void)hipFree(d_counter_);
    (void)hipHostFree(h_stage_);
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
    (void)hipHostFree(h_ring_);
    (void)hipHostFree(h_ready_);
    (void)hipHostFree(h_out_);
    for (auto &w : ws_win_) (void)hipFree(w);
    for (auto &e : ring_ev_)
        if (e) (void)hipEventDestroy(e);
    if (copy_done_) (void)hipEventDestroy(copy_done_);
    if (ws_ev_) (void)hipEventDestroy(ws_ev_);
    if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
    for (auto &ev : ev_)
        if (ev) (void)hipEventDestroy(ev);
    for (auto &slot : tev_)
        for (auto &ev : slot)
            if (ev) (void)hipEventDestroy(ev);
    if (own_stream_) (void)hipStreamDestroy(own_stream_);
    for (auto &ev : scan_ev_)
        if (ev) (void)hipEventDestroy(ev);
    if (res_ev_) (void)hipEventDestroy(res_ev_);
    for (auto &ev : res_done_)
        if (ev) (void)hipEventDestroy(ev);
    if (res_stream_) (void)hipStreamDestroy(res_stream_);
}

int Engine::set_gear(const uint64_t *gear) {
    if (!gear) {
        set_error("gear is NULL");
        return CDC_EINVAL;
    }
    if (in_flight()) {  // the batches in flight finish with the table they were submitted with
        const int64_t r = drain_implicit();
        if (r < 0) return (int)r;
    }
    if (wr_.active) {  // windows already chunked used the old table: a write never mixes two
        set_error("cdc_set_gear: a streaming write is in progress (cdc_write_finish it first)");
        return CDC_EINVAL;
    }
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipMemcpy(d_gear_, gear, 256 * sizeof(uint64_t), hipMemcpyHostToDevice));
    return CDC_OK;
}

size_t Engine::estimate(size_t len) const {
    if (algo_ == CDC_ALGO_FIXED) return len / min_ + 1;  // fixed_size.rs:45-47
    if (algo_ == CDC_ALGO_SEQ) return len / avg_;        // seq.rs:52-54
    return len / min_;  // fast.rs:47-49, rabin.rs:53-55, ultra.rs:41-43, leap.rs:41-43
}

size_t Engine::batch_max_chunks(size_t n, const uint64_t *lens) const {
    size_t t = 0;
    for (size_t i = 0; i < n; ++i) t += lens[i] / min_chunk() + 1;
    return t;
}

int Engine::ensure_host_staging(size_t n) {
    if (h_stage_ && h_stage_streams_ >= n) return CDC_OK;
    if (fb_any_) {  // (the batches in flight read their slots)
        set_error("internal: host staging regrown with FastCDC batches in flight");
        return CDC_EINVAL;
    }
    (void)hipHostFree(h_stage_);
    h_stage_ = nullptr;
    const size_t want = n + 64;
    // Per slot: ptrs[W] lens[W] span_base[W] tails[W] | stats ++ first[n+1]
    // (fixed: first[n+1]) -- stream tables 4 n, device-written stats ++
    // first[n+1] (n + 32).  Slots 1-2: more FastCDC batches in flight.
    h_stage_per_ = 5 * want + 32;
    HIP_TRY(placement().host_malloc(&h_stage_, kHostSlots * h_stage_per_ * sizeof(uint64_t), hipHostMallocCoherent));
    h_stage_streams_ = want;
    uint64_t *h = static_cast<uint64_t *>(h_stage_);
    fixed_tab_.h_ptrs = h;
    fixed_tab_.h_lens = h + want;
    fixed_tab_.h_sb = h + 2 * want;
    for (int k = 0; k < kSlots; ++k) fs_[k].tables.clear();
    return CDC_OK;
}

int Engine::ensure_workspace(uint64_t spans, size_t n) {
    if (ws_ && spans <= ws_spans_ && n <= ws_streams_) return CDC_OK;
    const uint64_t S = spans > ws_spans_ ? spans + spans / 4 + 16 : ws_spans_;
    const size_t N = n > ws_streams_ ? n + 64 : ws_streams_;
    const uint64_t cap = algo_ == CDC_ALGO_FASTCDC ? cap_ : 0;
    const uint64_t smax = algo_ == CDC_ALGO_FASTCDC ? smax_ : 0;
    const size_t A = 256;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, A);
        return o;
    };
    if (fb_any_) {
        set_error("internal: workspace regrown with FastCDC batches in flight");
        return CDC_EINVAL;
    }
    size_t o_count[kSlots], o_pos[kSlots], o_ptrs[kSlots], o_lens[kSlots], o_sb[kSlots], o_stats[kSlots],
        o_tails[kSlots];
    for (int k = 0; k < kSlots; ++k) {  // per batch in flight (FastCDC); the fixed-size path uses slot 0
        o_count[k] = take(S * 4);
        o_pos[k] = take(S * cap * 4);
        o_ptrs[k] = take(N * 8);
        o_lens[k] = take(N * 8);
        o_sb[k] = take((N + 1) * 8);
        o_stats[k] = take(p3::kStatWords * 8);
        o_tails[k] = take(N * 8);
    }
    const size_t o_starts = take(S * smax * 8);  // chunk starts beyond the LDS-resident ones
    const size_t o_first = take((N + 1) * 8);
    const uint64_t nb = p3::resolve_blocks(S) + 2;
    const size_t o_desc = take(6 * nb * 8);
    (void)hipFree(ws_);
    ws_ = nullptr;
    ws_spans_ = 0;
    ws_streams_ = 0;
    HIP_TRY(hipMalloc(&ws_, off));
    ++ws_gen_;
    ws_spans_ = S;
    ws_streams_ = N;
    char *b = static_cast<char *>(ws_);
    for (int k = 0; k < kSlots; ++k) {
        FastSlot &f = fs_[k];
        f.cand.cap = (uint32_t)cap;
        f.cand.count = reinterpret_cast<uint32_t *>(b + o_count[k]);
        f.cand.pos = reinterpret_cast<uint32_t *>(b + o_pos[k]);
        f.d_ptrs = reinterpret_cast<const uint8_t **>(b + o_ptrs[k]);
        f.d_lens = reinterpret_cast<uint64_t *>(b + o_lens[k]);
        f.d_sb = reinterpret_cast<uint64_t *>(b + o_sb[k]);
        f.d_tails = reinterpret_cast<uint64_t *>(b + o_tails[k]);
        f.stats = reinterpret_cast<uint64_t *>(b + o_stats[k]);
        f.tables.clear();
    }
    cand_ = fs_[0].cand;
    d_first_ = reinterpret_cast<uint64_t *>(b + o_first);
    fixed_tab_.d_ptrs = fs_[0].d_ptrs;
    fixed_tab_.d_lens = fs_[0].d_lens;
    fixed_tab_.d_sb = fs_[0].d_sb;
    ch3_.smax = (uint32_t)smax;
    ch3_.starts = reinterpret_cast<uint64_t *>(b + o_starts);
    uint64_t *desc = reinterpret_cast<uint64_t *>(b + o_desc);
    rs3_ = p3::Resolve{desc, desc + nb, desc + 2 * nb, desc + 3 * nb, desc + 4 * nb, desc + 5 * nb, 0};
    HIP_TRY(hipMemset(desc, 0, 6 * nb * 8));  // no stale status word can carry a live generation
    // The fill runs on the null stream, which the non-blocking streams the
    // kernels are launched on are not ordered against: it must have landed
    // before the first resolve publishes a status word.
    HIP_TRY(hipStreamSynchronize(nullptr));
    return CDC_OK;
}

int64_t Engine::chunk_batch_device(size_t n, const uint8_t *const *d_streams,
                                   const uint64_t *lens, cdc_chunk_t *d_out,
                                   size_t out_cap, uint64_t *first,
                                   hipStream_t stream) {
    return batch_device(n, d_streams, lens, d_out, out_cap, first, stream, false);
}

int64_t Engine::chunk_batch_device_async(size_t n, const uint8_t *const *d_streams, const uint64_t *lens,
                                         cdc_chunk_t *d_out, size_t out_cap, uint64_t *first,
                                         hipStream_t stream) {
    return batch_device(n, d_streams, lens, d_out, out_cap, first, stream, true);
}

int64_t Engine::batch_sync() {
    HIP_TRY(hipSetDevice(device_));
    if (in_flight()) {
        held_valid_ = false;
        return drain();
    }
    if (held_valid_) {  // an implicit drain already completed them: its result
        held_valid_ = false;
        return held_;
    }
    return 0;
}

// A drain that another call makes on the caller's behalf (any call on the
// handle completes the async batches first): its result -- the last batch's
// chunk count, or the error of a failed collection -- is what the next
// cdc_batch_sync returns.
int64_t Engine::drain_implicit() {
    if (!in_flight()) return 0;
    held_ = drain();
    held_valid_ = true;
    return held_;
}

bool Engine::in_flight() const { return fb_any_ || (walk_ && walk_->in_flight()); }

int Engine::walk_params(uint64_t *v, size_t n) const { return walk_ ? walk_->debug_params(v, n) : -1; }

int64_t Engine::drain() {
    if (!is_walk()) return fast_drain();
    const int64_t r = walk_->drain();
    timing_ = walk_->timing();  // (the last batch's, from its context)
    return r;
}

int64_t Engine::batch_device(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                             size_t out_cap, uint64_t *first, hipStream_t stream, bool async) {
    if (n && (!d_streams || !lens || !first)) {
        set_error("cdc_chunk_batch_device: NULL argument");
        return CDC_EINVAL;
    }
    if (n > 0xFFFFFFFEull) {
        set_error("too many streams");
        return CDC_EINVAL;
    }
    HIP_TRY(hipSetDevice(device_));
    hipStream_t s = stream ? stream : own_stream_;
    uint64_t bytes = 0, need = 0;
    for (size_t i = 0; i < n; ++i) {
        bytes += lens[i];
        need += lens[i] / min_chunk() + 1;
        if (lens[i] && !d_streams[i]) {
            set_error("NULL stream pointer with non-zero length");
            return CDC_EINVAL;
        }
        // Every content-defined kernel reads streams with 16-byte vector loads
        // (FastCDC scan, walk-engine bitmap pass and LDS windows).
        if (lens[i] && algo_ != CDC_ALGO_FIXED && (reinterpret_cast<uintptr_t>(d_streams[i]) & 15)) {
            set_error("device stream pointers must be 16-byte aligned");
            return CDC_EINVAL;
        }
    }
    if (need > out_cap) {
        set_error("out_cap < cdc_batch_max_chunks()");
        return CDC_EINVAL;
    }
    // Multi-megabyte async batches go to the walk contexts or into the
    // FastCDC pipeline; everything else runs to completion here, after the
    // batches in flight.
    if (is_walk()) {
        if (async && walk_->takes_async(n, bytes))
            return walk_->submit(n, d_streams, lens, d_out, out_cap, first, s, placement());
        if (in_flight()) {
            const int64_t r = drain_implicit();
            if (r < 0) return r;
        }
        const int64_t r = walk_->chunk_batch(n, d_streams, lens, d_out, out_cap, first, s, placement());
        const double hash_ms = timing_.hash_ms;  // (reported with the batch it hashed)
        timing_ = walk_->timing();
        timing_.hash_ms = hash_ms;
        return r;
    }
    const bool pipe = algo_ == CDC_ALGO_FASTCDC && n > 0 && bytes > kSmallBatch;
    if (!pipe && in_flight()) {
        const int64_t r = drain_implicit();
        if (r < 0) return r;
    }
    if (pipe) {
        // (async batches: the start / split / end events that cdc_last_timing
        // reads are recorded on every event_every_-th batch only -- each
        // event costs the stream ~4 us, r05t)
        const int64_t r = fast_submit(n, d_streams, lens, d_out, out_cap, first, bytes, s,
                                      !async || fb_seq_ % event_every_ == 0, async && two_stream_on_);
        if (r < 0 || async) return r;
        return fast_drain();
    }
    const double hash_ms = timing_.hash_ms;  // (reported with the batch it hashed)
    timing_pending_ = false;                 // (a new batch re-records the events)
    timing_ = cdc_timing_t{};
    timing_.hash_ms = hash_ms;
    timing_.bytes = bytes;
    timing_.path = CDC_PATH_EMPTY;
    if (n == 0) {
        if (first) first[0] = 0;
        return 0;
    }
    int rc = ensure_host_staging(n);
    if (rc) return rc;
    if (algo_ == CDC_ALGO_FASTCDC && n == 1 && !small_skip_ && small_ok(lens[0])) {
        rc = run_small(d_streams[0], lens[0], d_out, out_cap, first, s);
        if (rc == CDC_OK) {
            timing_.path = CDC_PATH_SMALL;  // (no events on the call path: timed stays 0)
            return (int64_t)first[1];
        }
        if (rc < 0) return rc;
        // (kSmallFallback: the regular pipeline below)
    }
    if (algo_ == CDC_ALGO_FASTCDC) {  // small batches: one scan + resolve, waited for here
        const int64_t r = fast_submit(n, d_streams, lens, d_out, out_cap, first, bytes, s, true, false);
        if (r < 0) return r;
        return fast_drain();
    }
    // Fixed-size: the streams own no spans; tables in staging slot 0.
    fixed_tab_.fill(n, d_streams, lens, 0);
    rc = ensure_workspace(0, n);
    if (rc) return rc;
    StreamTable st;
    rc = fixed_tab_.publish(n, bytes, 0, 0, ws_gen_, s, st);
    if (!rc) rc = run_fixed(st, n, lens, d_out, first, s);
    if (rc) return rc;
    return (int64_t)first[n];
}

// One FastCDC batch enqueued: its tables into the batch's slots, the scan and
// the resolve launches; no host wait.  The host collects it (fast_collect)
// when its stats block is needed again or at fast_drain().
int64_t Engine::fast_submit(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                            size_t out_cap, uint64_t *first, uint64_t bytes, hipStream_t s, bool timed, bool two_stream) {
    if (fb_any_ && (s != fb_stream_ || two_stream != fb_two_stream_)) {  // one pipeline per stream (pair)
        const int64_t r = drain_implicit();
        if (r < 0) return r;
    }
    if (two_stream && !res_stream_) {
        HIP_TRY(hipStreamCreateWithFlags(&res_stream_, hipStreamNonBlocking));
        for (auto &ev : scan_ev_) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&res_ev_, hipEventDisableTiming));
        for (auto &ev : res_done_) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (!std::getenv("CHUNKFS_AMD_NO_PREWARM")) {
            // The first ~100 two-stream batches of a process ran 10-20 % slower
            // than later ones, whichever handle ran them (profiles/r06/r06y_*):
            // the cross-stream event pattern, rehearsed once here with 4-byte
            // fills.
            void *d = nullptr;
            HIP_TRY(hipMalloc(&d, 256));
            for (int i = 0; i < 256; ++i) {
                HIP_TRY(hipMemsetAsync(d, i, 4, s));
                HIP_TRY(hipEventRecord(scan_ev_[i % kSlots], s));
                HIP_TRY(hipStreamWaitEvent(res_stream_, scan_ev_[i % kSlots], 0));
                HIP_TRY(hipMemsetAsync(static_cast<char *>(d) + 128, i, 4, res_stream_));
                HIP_TRY(hipEventRecord(res_done_[i % 3], res_stream_));
            }
            HIP_TRY(hipStreamSynchronize(res_stream_));
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(hipFree(d));
        }
    }
    const uint32_t sl2 = bytes <= kSmallBatch ? small_span_log2_ : span_log2_;
    uint64_t spans = 0;
    for (size_t i = 0; i < n; ++i) spans += (lens[i] + (1ull << sl2) - 1) >> sl2;
    const bool zero_copy = bytes <= kSmallBatch && n <= kZeroCopyStreams;
    const bool grow = !(h_stage_ && h_stage_streams_ >= n) || !(ws_ && spans <= ws_spans_ && n <= ws_streams_);
    if (fb_any_ && (zero_copy || grow)) {  // (buffers the batches in flight use)
        const int64_t r = drain_implicit();
        if (r < 0) return r;
    }
    const uint64_t seq = fb_seq_;
    if (fb_[seq % 3].live) {  // batch seq-3: its host block is this batch's
        const int rc = fast_collect((int)(seq % 3));
        if (rc) {
            (void)fast_drain();
            return rc;
        }
    }
    int rc = ensure_host_staging(n);
    if (rc) return rc;
    rc = ensure_workspace(spans ? spans : 1, n);
    if (rc) return rc;
    const int slot = (int)(seq % kSlots);
    FastSlot &f = fs_[slot];
    uint64_t *hb = static_cast<uint64_t *>(h_stage_) + (seq % kHostSlots) * h_stage_per_;
    uint64_t *h_ptrs = hb, *h_lens = hb + h_stage_streams_, *h_sb = hb + 2 * h_stage_streams_;
    uint64_t *h_tails = hb + 3 * h_stage_streams_;
    bool same = !zero_copy && f.tables_gen == ws_gen_ && f.tables.size() == 2 * n;
    for (size_t i = 0; same && i < n; ++i)
        same = f.tables[i] == reinterpret_cast<uint64_t>(d_streams[i]) && f.tables[n + i] == lens[i];
    {
        // this batch's tables in its own host block (its collection reads the
        // lengths); the device slot's copies are re-uploaded when they differ
        uint64_t sp = 0;
        uint32_t nt = 0;
        for (size_t i = 0; i < n; ++i) {
            h_ptrs[i] = reinterpret_cast<uint64_t>(d_streams[i]);
            h_lens[i] = lens[i];
            h_sb[i] = sp;
            sp += (lens[i] + (1ull << sl2) - 1) >> sl2;
            if (lens[i] & ((1ull << sl2) - 1)) h_tails[nt++] = sp - 1;  // ragged last span
        }
        h_sb[n] = sp;
        if (same && nt != f.n_tails) same = false;  // (cannot differ for equal tables; a guard)
        f.n_tails = nt;
    }
    if (!same) {
        f.tables.clear();
        if (!zero_copy) {
            HIP_TRY(hipMemcpyAsync(f.d_ptrs, h_ptrs, n * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(f.d_lens, h_lens, n * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(f.d_sb, h_sb, (n + 1) * 8, hipMemcpyHostToDevice, s));
            if (f.n_tails) HIP_TRY(hipMemcpyAsync(f.d_tails, h_tails, f.n_tails * 8, hipMemcpyHostToDevice, s));
            f.tables.assign(h_ptrs, h_ptrs + n);
            f.tables.insert(f.tables.end(), h_lens, h_lens + n);
            f.tables_gen = ws_gen_;
        }
    }
    StreamTable st{};
    st.ptrs = zero_copy ? reinterpret_cast<const uint8_t *const *>(h_ptrs) : f.d_ptrs;
    st.lens = zero_copy ? h_lens : f.d_lens;
    st.span_base = zero_copy ? h_sb : f.d_sb;
    st.n = (uint32_t)n;
    st.span_log2 = sl2;
    st.total_spans = spans;
    uint64_t *h_misc = hb + 4 * h_stage_streams_;  // stats ++ first[n+1], written by the device
    const p3::Compact cp{f.stats, h_misc, h_misc + p3::kStatWords};
    h_misc[p3::kStatDone] = ~0ull;  // sentinel: overwritten by the resolve's last block
    if (!spans) {  // every stream is empty: nothing to launch
        h_misc[p3::kStatDone] = 1;
        h_misc[p3::kStatError] = 0;
        for (size_t i = 0; i <= n; ++i) cp.h_first[i] = 0;
    }
    p3::Resolve rs = rs3_;
    rs.gen = ++res_gen_;
    FastBatch &rec = fb_[seq % 3];
    rec = FastBatch{};  // (live only once every launch is enqueued, below)
    rec.resolved = true;
    rec.two_stream = two_stream;
    rec.slot = slot;
    rec.h = hb;
    rec.n = n;
    rec.first = first;
    rec.seq = seq;
    rec.bytes = bytes;
    rec.spans = spans;
    hipEvent_t *ev = tev_[seq % kTimeRing];
    tev_timed_[seq % kTimeRing] = timed;
    rec.timed = timed;
    if (timed) HIP_TRY(hipEventRecord(ev[0], s));
    if (!two_stream) {
        if (spans)
            HIP_TRY(p3::launch_scan(st, fp_, d_gear_, f.cand, cp, zero_copy ? h_tails : f.d_tails, f.n_tails,
                                    num_cus_, s));
        if (timed) HIP_TRY(hipEventRecord(ev[1], s));
        if (spans) HIP_TRY(p3::launch_resolve(st, fp_, d_gear_, f.cand, ch3_, cp, rs, d_out, out_cap, s));
        if (timed) HIP_TRY(hipEventRecord(ev[2], s));
    } else {
        // The resolve goes to the second stream behind this scan's event, so
        // it runs beside the NEXT batch's scan.  Resolves stay in order
        // on that stream (the look-back descriptors and the spilled chunk
        // starts are shared).  No wait guards the device slot: its previous
        // user, batch seq - kSlots, is complete -- batch seq - kHostSlots was
        // collected above (or by a drain), and resolves retire in order.
        static_assert(kSlots > kHostSlots, "device slots must outlast the host blocks");
        if (spans)
            HIP_TRY(p3::launch_scan(st, fp_, d_gear_, f.cand, cp, zero_copy ? h_tails : f.d_tails, f.n_tails,
                                    num_cus_, s));
        if (timed) HIP_TRY(hipEventRecord(ev[1], s));
        HIP_TRY(hipEventRecord(scan_ev_[slot], s));
        HIP_TRY(hipStreamWaitEvent(res_stream_, scan_ev_[slot], 0));
        if (spans) HIP_TRY(p3::launch_resolve(st, fp_, d_gear_, f.cand, ch3_, cp, rs, d_out, out_cap, res_stream_));
        if (timed) HIP_TRY(hipEventRecord(ev[2], res_stream_));
        // (an untimed batch's own end marker on the resolve stream, where an
        // event costs the scans nothing: a slow collection waits for this
        // batch, not for the later resolves already queued behind it)
        else HIP_TRY(hipEventRecord(res_done_[seq % 3], res_stream_));
    }
    rec.live = true;
    fb_seq_ = seq + 1;
    fast_batches_ = fb_seq_;
    fb_any_ = true;
    fb_stream_ = s;
    fb_two_stream_ = two_stream;
    cand_ = f.cand;
    last_spans_ = spans;
    return 0;
}

// Every batch in flight collected in order.  Returns the last batch's chunk
// count.
int64_t Engine::fast_drain() {
    if (!fb_any_) return 0;
    const uint64_t last = fb_seq_ - 1;
    int rc = CDC_OK;
    int64_t total = 0;
    for (uint64_t q = last >= 2 ? last - 2 : 0; q <= last; ++q) {
        FastBatch &b = fb_[q % 3];
        if (!b.live || b.seq != q) continue;
        const int r = rc ? rc : fast_collect((int)(q % 3));
        b.live = false;
        if (r && !rc) rc = r;
        if (q == last && !rc) total = (int64_t)b.first[b.n];
    }
    if (fb_two_stream_) {
        // later work on the caller's stream is ordered after the resolves
        if (!rc && hipEventRecord(res_ev_, res_stream_) == hipSuccess)
            (void)hipStreamWaitEvent(fb_stream_, res_ev_, 0);
        else
            (void)hipStreamSynchronize(res_stream_);
    }
    if (rc) (void)hipStreamSynchronize(fb_stream_);  // (nothing of a failed pipeline stays in flight)
    fb_any_ = false;
    return rc ? rc : total;
}

// Wait for batch record k's resolve (its last block writes the done word into
// coherent pinned memory after a system-scope fence: spin on it, then the
// batch's end event), check it and hand first[] to the caller.
int Engine::fast_collect(int k) {
    FastBatch &b = fb_[k];
    if (!b.resolved) {
        set_error("internal: FastCDC batch collected before its resolve was enqueued");
        return CDC_EDEVICE;
    }
    uint64_t *h_misc = b.h + 4 * h_stage_streams_;
    {
        const volatile uint64_t *done = h_misc + p3::kStatDone;
        // (two streams: a batch's resolve runs after the NEXT batch's scan, so
        // its done word comes about a step later)
        const uint64_t us = b.two_stream ? std::min<uint64_t>(4000, std::max<uint64_t>(200, b.bytes / 1000000))
                                         : std::min<uint64_t>(2000, std::max<uint64_t>(100, b.bytes / 2000000));
        const auto budget = std::chrono::microseconds(us);
        const auto t_spin = std::chrono::steady_clock::now();
        while (*done == ~0ull && std::chrono::steady_clock::now() - t_spin < budget) __builtin_ia32_pause();
    }
    if (h_misc[p3::kStatDone] == ~0ull) {  // (slow batch or a failure: wait for the stream itself)
        if (b.timed) HIP_TRY(hipEventSynchronize(tev_[b.seq % kTimeRing][2]));
        else if (b.two_stream) HIP_TRY(hipEventSynchronize(res_done_[b.seq % 3]));
        else HIP_TRY(hipStreamSynchronize(fb_stream_));
    }
    b.live = false;
    if (h_misc[p3::kStatDone] != 1 || h_misc[p3::kStatError] != 0) {
        set_error(h_misc[p3::kStatDone] != 1 ? "resolve kernel did not report back"
                                             : "chain overflow, output bound or look-back timeout (internal error)");
        return CDC_EDEVICE;
    }
    if (fp_.diag & 64) {  // resolve block spans (100 MHz stamps -> us)
        const uint64_t *d = h_misc + p3::kStatDiag0;
        const uint64_t s0 = ~d[0], s1 = d[1], e1 = d[2], e0 = ~d[3];
        const double blocks = (double)p3::resolve_blocks(b.spans);
        std::fprintf(stderr, "resolve blocks, us: scan's last block end -> first start %.2f  starts spread %.2f  "
                             "first start -> first end %.2f  -> last end %.2f  longest block %.2f  mean block %.2f\n",
                     ((double)s0 - (double)d[6]) / 100.0, (s1 - s0) / 100.0, (e0 - s0) / 100.0, (e1 - s0) / 100.0,
                     d[4] / 100.0, d[5] / 100.0 / (blocks ? blocks : 1.0));
    } else if (fp_.diag & 128) {
        const double waves = (double)p3::resolve_blocks(b.spans) * 8;
        std::fprintf(stderr, (fp_.diag & 8192) ? "resolve link passes, us per wave (records: issue trunc link; "
                                                 "virtual: issue trunc link; -; -):"
                                               : "resolve phases, us per wave (meta recs settle+wait virtual-links "
                                                 "record-links walk lookback(w0) out):");
        for (int i = 0; i < p3::kStatDiagN; ++i)
            std::fprintf(stderr, " %.2f", (double)h_misc[p3::kStatDiag0 + i] / 100.0 / (waves ? waves : 1.0));
        std::fprintf(stderr, "\n");
    }
    // Zero-length streams own no span: their first[] is the next stream's.
    const uint64_t *lens = b.h + h_stage_streams_;
    uint64_t *hf = h_misc + p3::kStatWords;
    for (size_t i = b.n; i-- > 0;)
        if (lens[i] == 0) hf[i] = hf[i + 1];
    std::memcpy(b.first, hf, (b.n + 1) * 8);
    const double hash_ms = timing_.hash_ms;
    timing_ = cdc_timing_t{};
    timing_.hash_ms = hash_ms;
    timing_.bytes = b.bytes;
    timing_.candidates = h_misc[p3::kStatCand];
    timing_.overflow_spans = (uint32_t)h_misc[p3::kStatOvf];
    timing_.fixup_iterations = (uint32_t)h_misc[p3::kStatRewalk];
    timing_.walk_fallback_steps = h_misc[p3::kStatOnDemand];
    timing_.path = CDC_PATH_PIPELINE;
    timing_.timed = b.timed ? 1u : 0u;
    timing_pending_ = true;
    timing_seq_ = b.seq;
    return CDC_OK;
}

bool Engine::small_ok(uint64_t len) const {
    // ~len / 2^pmin records expected: keep well inside the kernel's record budget
    return small_on_ && len > 0 && len <= small::kMaxBytes && (len >> small_pmin_) <= small::kRecCap * 5 / 8;
}

int Engine::run_small(const uint8_t *data, uint64_t len, cdc_chunk_t *d_out, size_t out_cap, uint64_t *first,
                      hipStream_t s, bool host_input, const uint8_t *feed_src, uint8_t *feed_dst,
                      uint32_t feed_slot) {
    if (!small_mem_) {
        HIP_TRY(hipMalloc(&small_mem_, small::scratch_bytes() + small::copy_bytes() + small::bstamp_bytes()));
        // The ticket starts at 0.  On the launch's own stream: a fill on the
        // null stream is not ordered against a non-blocking stream, and one
        // that landed late would zero records the blocks have published.
        HIP_TRY(hipMemsetAsync(small_mem_, 0, small::scratch_bytes(), s));
        uint32_t *b = static_cast<uint32_t *>(small_mem_);
        small_ws_.brec = reinterpret_cast<uint64_t *>(b);
        small_ws_.bcnt = b + 2 * small::kMaxBlocks * small::kBlockRecCap;
        small_ws_.ticket = small_ws_.bcnt + small::kMaxBlocks;
        small_ws_.stamp = reinterpret_cast<uint64_t *>(static_cast<char *>(small_mem_) + small::scratch_bytes() - 64);
        small_ws_.bpub = small_ws_.stamp - small::kMaxBlocks;
        small_ws_.copy = static_cast<uint8_t *>(small_mem_) + small::scratch_bytes();
        small_ws_.bstamp = reinterpret_cast<uint64_t *>(small_ws_.copy + small::copy_bytes());
    }
    uint64_t *h = static_cast<uint64_t *>(h_stage_);
    uint64_t *h_misc = h + 4 * h_stage_streams_;  // (the regular path's stats ++ first[] area)
    uint64_t *h_first = h_misc + p3::kStatWords;
    volatile uint64_t *done = h_misc + small::kWordDone;
    *done = 0;
    small_seq_ = small_seq_ % 0xFFFFFFFEull + 1;  // 1 .. 2^32 - 2 (tags: seq << 32 | count)
    const small::Feed feed{feed_src ? h_ready_dev_ + (size_t)feed_slot * small::kFeedPieces : nullptr, small_seq_};
    auto feed_copy = [&]() {
        const auto tc = std::chrono::steady_clock::now();
        volatile uint64_t *ready = h_ready_ + (size_t)feed_slot * small::kFeedPieces;
        if (small_feed_pool_) {
            // the calling thread and whichever copy-pool helpers are awake
            // claim the pieces (work stealing: never a wait for a sleeper)
            pool_->copy_feed(feed_dst, feed_src, len, size_t(1) << small::kFeedLog2, ready, small_seq_);
        } else {
            // (A/B: the calling thread alone)
            const uint64_t piece = 1ull << small::kFeedLog2;
            for (uint64_t off = 0; off < len; off += piece) {
                std::memcpy(feed_dst + off, feed_src + off, std::min(piece, len - off));
                std::atomic_thread_fence(std::memory_order_release);  // (x86: stores stay in order)
                ready[off >> small::kFeedLog2] = small_seq_;
            }
        }
        small_copy_s_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - tc).count();
    };
    if (feed_src && small_feed_ == 2) feed_copy();  // (A/B: the feed copy first)
    HIP_TRY(small::launch_small(data, len, fp_, d_gear_, small_ws_, d_out, out_cap, h_misc, h_first, host_input,
                                feed, s));
    ++small_calls_;
    if (feed_src && small_feed_ != 2) {
        // The kernel is on its way (launch latency overlaps the copy): the
        // copy pool writes the bytes piece by piece, each announced by its
        // feed word once in memory.
        feed_copy();
    }
    // The last block writes the done word after a system-scope release: spin on
    // it (a call is ~20-60 us of device time), then the stream sync confirms.
    const auto t_spin = std::chrono::steady_clock::now();
    while (*done == 0 && std::chrono::steady_clock::now() - t_spin < std::chrono::microseconds(2000))
        __builtin_ia32_pause();
    if (*done == 0) HIP_TRY(hipStreamSynchronize(s));
    if (*done != 1) {
        set_error("small FastCDC kernel did not report back");
        return CDC_EDEVICE;
    }
    timing_pending_ = false;
    timing_.candidates = h_misc[small::kWordRecords];
    timing_.overflow_spans = 0;
    timing_.fixup_iterations = 0;
    timing_.walk_fallback_steps = 0;
    if (fp_.diag & small::kDiagStamps) {
        const uint64_t *t = h_misc + small::kWordStamp0;
        std::fprintf(stderr, "small: %llu B, us from block 0's start: last block %.2f, records %.2f, links %.2f "
                             "(%llu rounds), walk %.2f, output %.2f\n",
                     (unsigned long long)len, (t[1] - t[0]) / 100.0, (t[2] - t[0]) / 100.0, (t[3] - t[0]) / 100.0,
                     (unsigned long long)t[7], (t[4] - t[0]) / 100.0, (t[5] - t[0]) / 100.0);
        std::fprintf(stderr, "  round 0 max cycles per lane: load+trunc %llu, link %llu, successor %llu; rounds end at",
                     (unsigned long long)(t[6] & 0x1FFFFF), (unsigned long long)((t[6] >> 21) & 0x1FFFFF),
                     (unsigned long long)(t[6] >> 42));
        for (int k = 0; k < 4; ++k)
            if (h_first[2 + k]) std::fprintf(stderr, " %.2f", (h_first[2 + k] - t[0]) / 100.0);
        if (feed_src) std::fprintf(stderr, "; block 0 fed at %.2f; host copy %.2f us", (h_first[6] - t[0]) / 100.0,
                                   small_copy_s_ * 1e6);
        std::fprintf(stderr, "; round 0 added %llu entries, round 1 worked on %llu", (unsigned long long)(h_first[7] & 0xFFFF),
                     (unsigned long long)(h_first[7] >> 16));
        std::fprintf(stderr, "\n");
        // per-block stamps: min / median / max of start, fed, bytes in LDS, ticket
        const uint32_t G = (uint32_t)((len + small::kBlockBytes - 1) / small::kBlockBytes);
        std::vector<uint64_t> bs((size_t)G * 8);
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(bs.data(), small_ws_.bstamp, bs.size() * 8, hipMemcpyDeviceToHost));
        const char *nm[6] = {"fed", "loaded", "hashed(w0)", "tinfo(w0)", "drained", "ticket"};
        std::fprintf(stderr, "  blocks (%u):", G);
        for (int k = 0; k < 6; ++k) {
            std::vector<double> v;
            for (uint32_t b = 0; b < G; ++b) v.push_back(((double)bs[b * 8 + k] - (double)t[0]) / 100.0);
            std::sort(v.begin(), v.end());
            std::fprintf(stderr, " %s %.2f/%.2f/%.2f", nm[k], v.front(), v[v.size() / 2], v.back());
        }
        std::fprintf(stderr, "\n");
    }
    if (h_misc[small::kWordFallback]) {
        ++small_fallbacks_;
        return kSmallFallback;
    }
    first[0] = 0;
    first[1] = h_first[1];
    return CDC_OK;
}

// FastCDC batch events: [0] before its scan launch, [1] after it (before the
// resolve), [2] after the resolve.
const cdc_timing_t &Engine::timing() {
    if (in_flight()) (void)drain_implicit();  // (a failure is held for the next cdc_batch_sync)
    if (timing_pending_) {
        timing_pending_ = false;
        (void)timing_back((uint32_t)(fast_batches_ - 1 - timing_seq_), timing_);
    }
    return timing_;
}

int Engine::timing_back(uint32_t back, cdc_timing_t &out) {
    if (in_flight()) (void)drain_implicit();
    if (algo_ != CDC_ALGO_FASTCDC || back >= kTimeRing || back >= fast_batches_) {
        set_error("cdc_debug_timing_back: no such FastCDC batch in the event ring");
        return CDC_EINVAL;
    }
    if (&out != &timing_) out = timing_;
    hipEvent_t *ev = tev_[(fast_batches_ - 1 - back) % kTimeRing];
    float t01 = 0, t12 = 0, t02 = 0;
    HIP_TRY(hipSetDevice(device_));
    out.path = CDC_PATH_PIPELINE;
    out.timed = tev_timed_[(fast_batches_ - 1 - back) % kTimeRing] ? 1u : 0u;
    if (!out.timed) {  // an async batch recorded without events
        out.scan_ms = out.resolve_ms = out.total_ms = 0;
        return CDC_OK;
    }
    HIP_TRY(hipEventSynchronize(ev[2]));
    HIP_TRY(hipEventElapsedTime(&t01, ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&t12, ev[1], ev[2]));
    HIP_TRY(hipEventElapsedTime(&t02, ev[0], ev[2]));
    out.scan_ms = t01;
    out.resolve_ms = t12;
    out.total_ms = t02;
    return CDC_OK;
}

int Engine::run_fixed(const StreamTable &st, size_t n, const uint64_t *lens,
                      cdc_chunk_t *d_out, uint64_t *first, hipStream_t s) {
    uint64_t *h = static_cast<uint64_t *>(h_stage_);
    uint64_t *h_first = h + 4 * h_stage_streams_;
    uint64_t t = 0;
    for (size_t i = 0; i < n; ++i) {
        h_first[i] = t;
        t += (lens[i] + min_ - 1) / min_;  // fixed_size.rs:35-40: ceil(len/cs) chunks
    }
    h_first[n] = t;
    HIP_TRY(hipEventRecord(ev_[0], s));
    HIP_TRY(hipMemcpyAsync(d_first_, h_first, (n + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_fixed(st, min_, d_first_, d_out, t, s));
    HIP_TRY(hipEventRecord(ev_[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(first, h_first, (n + 1) * 8);
    float t03 = 0;
    HIP_TRY(hipEventElapsedTime(&t03, ev_[0], ev_[3]));
    timing_.total_ms = t03;
    timing_.scan_ms = t03;
    timing_.path = CDC_PATH_FIXED;
    timing_.timed = 1;
    return CDC_OK;
}

int64_t Engine::fs_write(const uint8_t *data, size_t len, size_t seg_size, std::vector<uint64_t> &spans,
                         double *seconds) {
    spans.clear();
    if (seg_size == 0) {
        set_error("cdc_fs_write: seg_size must be > 0");
        return CDC_EINVAL;
    }
    if (len && !data) {
        set_error("cdc_fs_write: data is NULL");
        return CDC_EINVAL;
    }
    // ChunkStorage::write (storage.rs:84-100): StorageWriter::write per
    // seg_size slice, then flush -- through the streaming write path.
    int rc = write_begin();
    if (rc) return rc;  // (e.g. a streaming write in progress: left alone)
    for (size_t off = 0; !rc && off < len; off += seg_size)
        rc = write_segment(data + off, std::min(seg_size, len - off));
    if (rc) {
        wr_.active = false;
        return rc;
    }
    return write_finish(spans, seconds);
}

int Engine::sha256_device(const uint8_t *d_data, const cdc_chunk_t *d_chunks, size_t n,
                          uint8_t *d_digests, hipStream_t s) {
    const uint64_t first[2] = {0, n};
    return sha256_batch(1, &d_data, first, d_chunks, d_digests, s);
}

// One launch over every chunk of every stream (sha256.hip); the stream table
// (first[], bases) goes up through a pinned block with one H2D copy.
int Engine::sha256_batch(size_t n, const uint8_t *const *d_streams, const uint64_t *first,
                         const cdc_chunk_t *d_chunks, uint8_t *d_digests, hipStream_t s) {
    if (n == 0) return CDC_OK;
    if (!d_streams || !first) {
        set_error("cdc_sha256_batch_device: NULL stream table");
        return CDC_EINVAL;
    }
    if (first[0] != 0) {
        set_error("cdc_sha256_batch_device: first[0] must be 0");
        return CDC_EINVAL;
    }
    for (size_t i = 0; i < n; ++i) {
        if (first[i + 1] < first[i]) {
            set_error("cdc_sha256_batch_device: first[] must be non-decreasing");
            return CDC_EINVAL;
        }
        if (first[i + 1] > first[i] && !d_streams[i]) {
            set_error("cdc_sha256_batch_device: NULL stream with chunks");
            return CDC_EINVAL;
        }
    }
    const uint64_t total = first[n];
    if (total >= (1ull << 32)) {
        set_error("cdc_sha256_batch_device: more than 2^32 - 1 chunks in one batch");
        return CDC_EINVAL;
    }
    if (total && (!d_chunks || !d_digests)) {
        set_error("cdc_sha256_chunks_device: NULL argument");
        return CDC_EINVAL;
    }
    HIP_TRY(hipSetDevice(device_));
    if (in_flight()) {  // (the chunks it hashes are usually the last batch's)
        const int64_t r = drain_implicit();
        if (r < 0) return (int)r;
    }
    hipStream_t st = s ? s : own_stream_;
    (void)timing();  // the last batch's events, before ev_[2] is re-recorded
    if (total == 0) {
        timing_.hash_ms = 0;
        return CDC_OK;
    }
    const size_t words = 2 * n + 1;
    if (sha_tab_cap_ < words) {
        (void)hipFree(d_sha_tab_);
        (void)hipHostFree(h_sha_tab_);
        d_sha_tab_ = h_sha_tab_ = nullptr;
        sha_tab_cap_ = 0;
        const size_t want = words + 64;
        HIP_TRY(hipMalloc(&d_sha_tab_, want * 8));
        HIP_TRY(hipHostMalloc(&h_sha_tab_, want * 8, hipHostMallocDefault));
        sha_tab_cap_ = want;
    }
    std::memcpy(h_sha_tab_, first, (n + 1) * 8);
    for (size_t i = 0; i < n; ++i) h_sha_tab_[n + 1 + i] = reinterpret_cast<uint64_t>(d_streams[i]);
    HIP_TRY(hipMemcpyAsync(d_sha_tab_, h_sha_tab_, words * 8, hipMemcpyHostToDevice, st));
    ShaBatch b{};
    b.chunks = reinterpret_cast<const cdc_chunk_pod *>(d_chunks);
    b.n_chunks = total;
    b.first = d_sha_tab_;
    b.base = d_sha_tab_ + n + 1;
    b.n_streams = (uint32_t)n;
    b.digests = reinterpret_cast<uint32_t *>(d_digests);
    b.counter = d_counter_;
    if (sha_order_cap_ < total) {
        (void)hipFree(d_sha_order_);
        d_sha_order_ = nullptr;
        sha_order_cap_ = 0;
        const uint64_t want = total + total / 8 + 1024;
        HIP_TRY(hipMalloc(&d_sha_order_, want * sizeof(uint32_t)));
        sha_order_cap_ = want;
    }
    b.order = d_sha_order_;
    HIP_TRY(hipEventRecord(ev_[3], st));
    HIP_TRY(launch_sha256(b, num_cus_, st));
    HIP_TRY(hipEventRecord(ev_[2], st));
    HIP_TRY(hipStreamSynchronize(st));  // (also: the pinned table may be rewritten by the next call)
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev_[3], ev_[2]));
    timing_.hash_ms = ms;
    return CDC_OK;
}

int64_t Engine::debug_copy(int what, void *out, size_t max_bytes) {
    if (in_flight()) {
        const int64_t r = drain_implicit();
        if (r < 0) return r;
    }
    if (algo_ != CDC_ALGO_FASTCDC || !ws_) {
        set_error("debug_copy: no FastCDC batch yet");
        return CDC_EINVAL;
    }
    const void *src = nullptr;
    size_t bytes = 0;
    if (what == 0) {
        src = cand_.count;
        bytes = last_spans_ * 4;
    } else if (what == 1) {
        src = cand_.pos;
        bytes = last_spans_ * cap_ * 4;
    } else {
        set_error("debug_copy: unknown array");
        return CDC_EINVAL;
    }
    if (bytes > max_bytes) bytes = max_bytes;
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipStreamSynchronize(own_stream_));
    if (bytes) HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return (int64_t)bytes;
}

int Engine::read_bw(const uint8_t *d_buf, size_t len, int reps, double *ms) {
    HIP_TRY(hipSetDevice(device_));
    if (in_flight()) {
        const int64_t r = drain_implicit();
        if (r < 0) return (int)r;
    }
    uint64_t *d_acc = nullptr;
    const size_t words = (size_t)num_cus_ * 8;
    HIP_TRY(hipMalloc(&d_acc, words * 8));
    hipError_t e = hipMemsetAsync(d_acc, 0, words * 8, own_stream_);
    if (e == hipSuccess) e = launch_read_reduce(d_buf, len, d_acc, num_cus_, own_stream_);  // (warm-up)
    if (e == hipSuccess) e = hipEventRecord(ev_[0], own_stream_);
    for (int r = 0; e == hipSuccess && r < reps; ++r) e = launch_read_reduce(d_buf, len, d_acc, num_cus_, own_stream_);
    if (e == hipSuccess) e = hipEventRecord(ev_[3], own_stream_);
    if (e == hipSuccess) e = hipEventSynchronize(ev_[3]);
    float t = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ev_[0], ev_[3]);
    (void)hipFree(d_acc);
    if (e != hipSuccess) {
        set_error(std::string("read_bw: ") + hipGetErrorString(e));
        return CDC_EDEVICE;
    }
    *ms = (double)t / reps;
    return CDC_OK;
}

int Engine::fill_splitmix64(uint8_t *d_buf, size_t len, uint64_t seed, hipStream_t s) {
    HIP_TRY(hipSetDevice(device_));
    hipStream_t st = s ? s : own_stream_;
    HIP_TRY(launch_fill_splitmix64(d_buf, len, seed, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CDC_OK;
}

// ---- Rabin / UltraCDC / LeapCDC / SeqCDC / AE handles (walk_engine.cpp) ----

int Engine::create_seq(const uint32_t seq[4], uint32_t min, uint32_t avg, uint32_t max, int device,
                       Engine **out) {
    if (!seq) {
        set_error("cdc_create_seq: config is NULL");
        return CDC_EINVAL;
    }
    WalkConfig cfg;
    cfg.seq_mode = seq[0];
    cfg.seq_length = seq[1];
    cfg.seq_jump_trigger = seq[2];
    cfg.seq_jump_size = seq[3];
    return create_walk(CDC_ALGO_SEQ, cfg, min, avg, max, device, out);
}

int Engine::create_ae(uint32_t mode, uint32_t window, uint32_t min, uint32_t avg, uint32_t max, int device,
                      Engine **out) {
    WalkConfig cfg;
    cfg.ae_mode = mode;
    cfg.ae_window = window;
    return create_walk(CDC_ALGO_AE, cfg, min, avg, max, device, out);
}

int Engine::create_walk(cdc_algo_t algo, WalkConfig &cfg, uint32_t min, uint32_t avg, uint32_t max, int device,
                        Engine **out) {
    if (!out) {
        set_error("cdc_create: out is NULL");
        return CDC_EINVAL;
    }
    *out = nullptr;
    std::string describe;
    int rc = WalkEngine::validate(algo, min, avg, max, cfg, describe);  // (before any HIP call)
    if (rc != CDC_OK) return rc;
    Engine *e = new Engine();
    e->algo_ = algo;
    e->min_ = min;
    e->avg_ = avg;
    e->max_ = max;
    e->device_ = device;
    e->describe_ = describe;
    rc = e->init();
    if (rc == CDC_OK) rc = WalkEngine::create(algo, min, avg, max, cfg, device, e->walk_);
    if (rc != CDC_OK) {
        delete e;
        return rc;
    }
    *out = e;
    return CDC_OK;
}

int Engine::set_rabin_poly(uint64_t P) {
    if (algo_ != CDC_ALGO_RABIN) {
        set_error("cdc_set_rabin_poly: not a RabinChunker handle");
        return CDC_EINVAL;
    }
    const int deg = P ? 63 - __builtin_clzll(P) : -1;
    if (deg < 9 || deg > 56) {
        set_error("cdc_set_rabin_poly: polynomial degree must be 9..56");
        return CDC_EINVAL;
    }
    if (wr_.active) {  // windows already chunked used the old polynomial: a write never mixes two
        set_error("cdc_set_rabin_poly: a streaming write is in progress (cdc_write_finish it first)");
        return CDC_EINVAL;
    }
    HIP_TRY(hipSetDevice(device_));
    if (in_flight()) {  // the batches in flight finish with the polynomial they were submitted with
        const int64_t r = drain_implicit();
        if (r < 0) return (int)r;
    }
    HIP_TRY(hipStreamSynchronize(own_stream_));
    return walk_->set_rabin_poly(P);
}

}  // namespace cdc
