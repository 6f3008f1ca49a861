// fast_engine.cpp -- host orchestration of the FastCDC kernels.
//
// Per pipeline batch (DESIGN.md "FastCDC: two kernels"):
//   H2D of the small per-stream tables (skipped when unchanged; small batches
//   read them from the pinned block itself) -> scan -> resolve (writes the
//   chunks to HBM and stats ++ first[n+1] straight into coherent pinned host
//   memory) -> the host spins on the batch's done word.
// Async batches keep up to three in flight, the resolves on a second stream.
// A single small stream goes to the one-launch kernel (small.hip) first.
#include "fast_engine.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/chunkfs_amd_tables.h"

namespace cdc {

namespace {
#ifndef CDC_MIN_SPAN_LOG2
#define CDC_MIN_SPAN_LOG2 16
#endif
constexpr uint32_t kMinSpanLog2 = CDC_MIN_SPAN_LOG2;  // 64 KiB spans at least (experiment builds may raise it)
constexpr uint32_t kMaxSpanLog2 = 17;  // ... and at most 128 KiB unless the max chunk needs more

// fastcdc 3.1.0 v2020 FastCDC::new asserts (VERIFY).
constexpr uint32_t kMinimumMin = 64, kMinimumMax = 1048576;
constexpr uint32_t kAverageMin = 256, kAverageMax = 4194304;
constexpr uint32_t kMaximumMin = 1024, kMaximumMax = 16777216;

// The Level1 mask pair of an average size.
void masks_of(uint32_t avg, uint64_t &mask_s, uint64_t &mask_l) {
    const unsigned bits = (unsigned)std::lround(std::log2((double)avg));
    mask_s = CHUNKFS_AMD_MASKS[bits + 1];
    mask_l = CHUNKFS_AMD_MASKS[bits - 1];
}
}  // namespace

int FastEngine::validate(uint32_t min, uint32_t avg, uint32_t max, std::string &describe) {
    if (min < kMinimumMin || min > kMinimumMax || avg < kAverageMin ||
        avg > kAverageMax || max < kMaximumMin || max > kMaximumMax) {
        set_error("FastCDC sizes out of range (fastcdc v2020 asserts: min 64..1MiB, "
                  "avg 256..4MiB, max 1KiB..16MiB)");
        return CDC_EINVAL;
    }
    // The rule has no defined answer below these orderings: with max < min
    // every chunk is max bytes, more than the len / min + 1 that the output
    // and the workspace are sized for; with max < avg the published first
    // loop runs to a centre past the clipped remainder.  (min > avg is
    // well defined: the first loop is empty.)
    if (max < min || max < avg) {
        set_error("FastCDC sizes out of order: max must be >= min and >= avg");
        return CDC_EINVAL;
    }
    uint64_t mask_s, mask_l;
    masks_of(avg, mask_s, mask_l);
    if (63 - (uint32_t)__builtin_clzll(mask_s | mask_l) > 47) {  // the 3-lane carry is exact mod 2^48 only
        set_error("mask tests bit >= 48: unsupported");
        return CDC_EINVAL;
    }
    char buf[256];
    std::snprintf(buf, sizeof buf,
                  "FastCDC (2020), sizes: SizeParams { min: %u, avg: %u, max: %u } "
                  "[MI355X gfx950]",
                  min, avg, max);
    describe = buf;
    return CDC_OK;
}

int FastEngine::create(uint32_t min, uint32_t avg, uint32_t max, int device, int num_cus,
                       std::unique_ptr<FastEngine> &out) {
    std::unique_ptr<FastEngine> e(new FastEngine());
    e->device_ = device;
    e->num_cus_ = num_cus;
    FastParams &fp = e->fp_;
    fp.min = min;
    fp.avg = avg;
    fp.max = max;
    masks_of(avg, fp.mask_s, fp.mask_l);
    fp.cmask = fp.mask_s & fp.mask_l;
    const uint64_t all = fp.mask_s | fp.mask_l;
    fp.trunc = 63 - (uint32_t)__builtin_clzll(all);
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
    for (auto &slot : e->tev_)
        for (auto &ev : slot) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipMalloc(&e->d_gear_, 256 * sizeof(uint64_t)));
    HIP_TRY(hipMemcpy(e->d_gear_, CHUNKFS_AMD_GEAR, 256 * sizeof(uint64_t), hipMemcpyHostToDevice));
    out = std::move(e);
    return CDC_OK;
}

FastEngine::~FastEngine() {
    if (any_) (void)drain();
    if (res_stream_) (void)hipStreamSynchronize(res_stream_);
    (void)hipFree(ws_);
    (void)hipFree(small_mem_);
    (void)hipFree(d_gear_);
    (void)hipHostFree(h_stage_);
    for (auto &slot : tev_)
        for (auto &ev : slot)
            if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : scan_ev_)
        if (ev) (void)hipEventDestroy(ev);
    if (res_ev_) (void)hipEventDestroy(res_ev_);
    for (auto &ev : res_done_)
        if (ev) (void)hipEventDestroy(ev);
    if (res_stream_) (void)hipStreamDestroy(res_stream_);
}

int FastEngine::set_gear(const uint64_t *gear) {
    HIP_TRY(hipMemcpy(d_gear_, gear, 256 * sizeof(uint64_t), hipMemcpyHostToDevice));
    return CDC_OK;
}

// Callers drain first: the batches in flight read their blocks.
int FastEngine::ensure_host_staging(size_t n, const HostPlacement &place) {
    if (h_stage_ && h_stage_streams_ >= n) return CDC_OK;
    (void)hipHostFree(h_stage_);
    h_stage_ = nullptr;
    h_stage_streams_ = 0;
    const size_t W = n + 64;
    // Per block: ptrs[W] lens[W] span_base[W] tails[W] | stats ++ first[n+1],
    // the last two written by the device.
    const size_t per = 5 * W + 2 * p3::kStatWords;
    HIP_TRY(place.host_malloc(&h_stage_, kHostSlots * per * sizeof(uint64_t), hipHostMallocCoherent));
    h_stage_streams_ = W;
    for (int k = 0; k < kHostSlots; ++k) {
        uint64_t *h = static_cast<uint64_t *>(h_stage_) + k * per;
        hb_[k] = HostBlock{h, h + W, h + 2 * W, h + 3 * W, h + 4 * W, h + 4 * W + p3::kStatWords};
    }
    for (auto &f : fs_) f.tables.clear();
    return CDC_OK;
}

// Callers drain first: the batches in flight use the arena.
int FastEngine::ensure_workspace(uint64_t spans, size_t n) {
    if (ws_ && spans <= ws_spans_ && n <= ws_streams_) return CDC_OK;
    const uint64_t S = spans > ws_spans_ ? spans + spans / 4 + 16 : ws_spans_;
    const size_t N = n > ws_streams_ ? n + 64 : ws_streams_;
    const size_t A = 256;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, A);
        return o;
    };
    size_t o_count[kSlots], o_pos[kSlots], o_ptrs[kSlots], o_lens[kSlots], o_sb[kSlots], o_stats[kSlots],
        o_tails[kSlots];
    for (int k = 0; k < kSlots; ++k) {  // per batch in flight
        o_count[k] = take(S * 4);
        o_pos[k] = take(S * cap_ * 4);
        o_ptrs[k] = take(N * 8);
        o_lens[k] = take(N * 8);
        o_sb[k] = take((N + 1) * 8);
        o_stats[k] = take(p3::kStatWords * 8);
        o_tails[k] = take(N * 8);
    }
    const size_t o_starts = take(S * smax_ * 8);  // chunk starts beyond the LDS-resident ones
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
        f.cand.cap = cap_;
        f.cand.count = reinterpret_cast<uint32_t *>(b + o_count[k]);
        f.cand.pos = reinterpret_cast<uint32_t *>(b + o_pos[k]);
        f.d_ptrs = reinterpret_cast<const uint8_t **>(b + o_ptrs[k]);
        f.d_lens = reinterpret_cast<uint64_t *>(b + o_lens[k]);
        f.d_sb = reinterpret_cast<uint64_t *>(b + o_sb[k]);
        f.d_tails = reinterpret_cast<uint64_t *>(b + o_tails[k]);
        f.stats = reinterpret_cast<uint64_t *>(b + o_stats[k]);
        f.tables.clear();
    }
    ch3_.smax = smax_;
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

int64_t FastEngine::chunk_batch(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                                size_t out_cap, uint64_t *first, hipStream_t s, const HostPlacement &place,
                                bool skip_small, int64_t &drained) {
    drained = kNoDrain;
    uint64_t bytes = 0;
    for (size_t i = 0; i < n; ++i) bytes += lens[i];
    if (takes_async(n, bytes)) {  // a pipeline batch, behind the ones in flight where it can be
        const int64_t r = enqueue(n, d_streams, lens, d_out, out_cap, first, bytes, s, place, true, false, drained);
        return r < 0 ? r : drain();
    }
    if (any_) {
        drained = drain();
        if (drained < 0) return drained;
    }
    timing_pending_ = false;  // (a new batch re-records the events)
    timing_ = cdc_timing_t{};
    timing_.bytes = bytes;
    timing_.path = CDC_PATH_EMPTY;
    if (n == 0) {
        if (first) first[0] = 0;
        return 0;
    }
    if (n == 1 && !skip_small && small_ok(lens[0])) {
        const int rc = run_small(d_streams[0], lens[0], d_out, out_cap, first, s, place);
        if (rc == CDC_OK) {
            timing_.path = CDC_PATH_SMALL;  // (no events on the call path: timed stays 0)
            return (int64_t)first[1];
        }
        if (rc < 0) return rc;
        // (kSmallFallback: the regular pipeline below)
    }
    // small batches: one scan + resolve, waited for here
    const int64_t r = enqueue(n, d_streams, lens, d_out, out_cap, first, bytes, s, place, true, false, drained);
    return r < 0 ? r : drain();
}

int64_t FastEngine::submit(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                           size_t out_cap, uint64_t *first, hipStream_t s, const HostPlacement &place,
                           int64_t &drained) {
    drained = kNoDrain;
    uint64_t bytes = 0;
    for (size_t i = 0; i < n; ++i) bytes += lens[i];
    return enqueue(n, d_streams, lens, d_out, out_cap, first, bytes, s, place, seq_ % event_every_ == 0,
                   two_stream_on_, drained);
}

// One batch enqueued: its tables into the batch's slot and block, the scan
// and the resolve launches; no host wait.  The host collects it (collect)
// when its host block is needed again or at drain().
int64_t FastEngine::enqueue(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                            size_t out_cap, uint64_t *first, uint64_t bytes, hipStream_t s,
                            const HostPlacement &place, bool timed, bool two_stream, int64_t &drained) {
    if (any_ && (s != stream_ || two_stream != any_two_stream_)) {  // one pipeline per stream (pair)
        drained = drain();
        if (drained < 0) return drained;
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
    if (any_ && (zero_copy || grow)) {  // (buffers the batches in flight use)
        drained = drain();
        if (drained < 0) return drained;
    }
    const uint64_t seq = seq_;
    if (fb_[seq % 3].live) {  // batch seq-3: its host block is this batch's
        const int rc = collect((int)(seq % 3));
        if (rc) {
            (void)drain();
            return rc;
        }
    }
    int rc = ensure_host_staging(n, place);
    if (rc) return rc;
    rc = ensure_workspace(spans ? spans : 1, n);
    if (rc) return rc;
    const int slot = (int)(seq % kSlots);
    FastSlot &f = fs_[slot];
    const HostBlock &h = hb_[seq % kHostSlots];
    bool same = !zero_copy && f.tables_gen == ws_gen_ && f.tables.size() == 2 * n;
    for (size_t i = 0; same && i < n; ++i)
        same = f.tables[i] == reinterpret_cast<uint64_t>(d_streams[i]) && f.tables[n + i] == lens[i];
    {
        // this batch's tables in its own host block (its collection reads the
        // lengths); the device slot's copies are re-uploaded when they differ
        uint64_t sp = 0;
        uint32_t nt = 0;
        for (size_t i = 0; i < n; ++i) {
            h.ptrs[i] = reinterpret_cast<uint64_t>(d_streams[i]);
            h.lens[i] = lens[i];
            h.sb[i] = sp;
            sp += (lens[i] + (1ull << sl2) - 1) >> sl2;
            if (lens[i] & ((1ull << sl2) - 1)) h.tails[nt++] = sp - 1;  // ragged last span
        }
        h.sb[n] = sp;
        if (same && nt != f.n_tails) same = false;  // (cannot differ for equal tables; a guard)
        f.n_tails = nt;
    }
    if (!same) {
        f.tables.clear();
        if (!zero_copy) {
            HIP_TRY(hipMemcpyAsync(f.d_ptrs, h.ptrs, n * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(f.d_lens, h.lens, n * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(f.d_sb, h.sb, (n + 1) * 8, hipMemcpyHostToDevice, s));
            if (f.n_tails) HIP_TRY(hipMemcpyAsync(f.d_tails, h.tails, f.n_tails * 8, hipMemcpyHostToDevice, s));
            f.tables.assign(h.ptrs, h.ptrs + n);
            f.tables.insert(f.tables.end(), h.lens, h.lens + n);
            f.tables_gen = ws_gen_;
        }
    }
    StreamTable st{};
    st.ptrs = zero_copy ? reinterpret_cast<const uint8_t *const *>(h.ptrs) : f.d_ptrs;
    st.lens = zero_copy ? h.lens : f.d_lens;
    st.span_base = zero_copy ? h.sb : f.d_sb;
    st.n = (uint32_t)n;
    st.span_log2 = sl2;
    st.total_spans = spans;
    const p3::Compact cp{f.stats, h.stats, h.first};
    h.stats[p3::kStatDone] = ~0ull;  // sentinel: overwritten by the resolve's last block
    if (!spans) {  // every stream is empty: nothing to launch
        h.stats[p3::kStatDone] = 1;
        h.stats[p3::kStatError] = 0;
        for (size_t i = 0; i <= n; ++i) h.first[i] = 0;
    }
    p3::Resolve rs = rs3_;
    rs.gen = ++res_gen_;
    FastBatch &rec = fb_[seq % 3];
    rec = FastBatch{};  // (live only once every launch is enqueued, below)
    rec.two_stream = two_stream;
    rec.slot = slot;
    rec.n = n;
    rec.first = first;
    rec.seq = seq;
    rec.bytes = bytes;
    rec.spans = spans;
    hipEvent_t *ev = tev_[seq % kTimeRing];
    tev_timed_[seq % kTimeRing] = timed;
    rec.timed = timed;
    const uint64_t *d_tails = zero_copy ? h.tails : f.d_tails;
    if (timed) HIP_TRY(hipEventRecord(ev[0], s));
    if (!two_stream) {
        if (spans) HIP_TRY(p3::launch_scan(st, fp_, d_gear_, f.cand, cp, d_tails, f.n_tails, num_cus_, s));
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
        if (spans) HIP_TRY(p3::launch_scan(st, fp_, d_gear_, f.cand, cp, d_tails, f.n_tails, num_cus_, s));
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
    seq_ = seq + 1;
    small_last_len_ = 0;
    any_ = true;
    stream_ = s;
    any_two_stream_ = two_stream;
    return 0;
}

int64_t FastEngine::drain() {
    if (!any_) return 0;
    const uint64_t last = seq_ - 1;
    int rc = CDC_OK;
    int64_t total = 0;
    for (uint64_t q = last >= 2 ? last - 2 : 0; q <= last; ++q) {
        FastBatch &b = fb_[q % 3];
        if (!b.live || b.seq != q) continue;
        const int r = rc ? rc : collect((int)(q % 3));
        b.live = false;
        if (r && !rc) rc = r;
        if (q == last && !rc) total = (int64_t)b.first[b.n];
    }
    if (any_two_stream_) {
        // later work on the caller's stream is ordered after the resolves
        if (!rc && hipEventRecord(res_ev_, res_stream_) == hipSuccess)
            (void)hipStreamWaitEvent(stream_, res_ev_, 0);
        else
            (void)hipStreamSynchronize(res_stream_);
    }
    if (rc) (void)hipStreamSynchronize(stream_);  // (nothing of a failed pipeline stays in flight)
    any_ = false;
    return rc ? rc : total;
}

// Wait for batch record k's resolve (its last block writes the done word into
// coherent pinned memory after a system-scope fence: spin on it, then the
// batch's end event), check it and hand first[] to the caller.
int FastEngine::collect(int k) {
    FastBatch &b = fb_[k];
    const HostBlock &h = hb_[k];
    {
        const volatile uint64_t *done = h.stats + p3::kStatDone;
        // (two streams: a batch's resolve runs after the NEXT batch's scan, so
        // its done word comes about a step later)
        const uint64_t us = b.two_stream ? std::min<uint64_t>(4000, std::max<uint64_t>(200, b.bytes / 1000000))
                                         : std::min<uint64_t>(2000, std::max<uint64_t>(100, b.bytes / 2000000));
        const auto budget = std::chrono::microseconds(us);
        const auto t_spin = std::chrono::steady_clock::now();
        while (*done == ~0ull && std::chrono::steady_clock::now() - t_spin < budget) __builtin_ia32_pause();
    }
    if (h.stats[p3::kStatDone] == ~0ull) {  // (slow batch or a failure: wait for the stream itself)
        if (b.timed) HIP_TRY(hipEventSynchronize(tev_[b.seq % kTimeRing][2]));
        else if (b.two_stream) HIP_TRY(hipEventSynchronize(res_done_[b.seq % 3]));
        else HIP_TRY(hipStreamSynchronize(stream_));
    }
    b.live = false;
    if (h.stats[p3::kStatDone] != 1 || h.stats[p3::kStatError] != 0) {
        set_error(h.stats[p3::kStatDone] != 1 ? "resolve kernel did not report back"
                                              : "chain overflow, output bound or look-back timeout (internal error)");
        return CDC_EDEVICE;
    }
    if (fp_.diag & 64) {  // resolve block spans (100 MHz stamps -> us)
        const uint64_t *d = h.stats + p3::kStatDiag0;
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
            std::fprintf(stderr, " %.2f", (double)h.stats[p3::kStatDiag0 + i] / 100.0 / (waves ? waves : 1.0));
        std::fprintf(stderr, "\n");
    }
    // Zero-length streams own no span: their first[] is the next stream's.
    for (size_t i = b.n; i-- > 0;)
        if (h.lens[i] == 0) h.first[i] = h.first[i + 1];
    std::memcpy(b.first, h.first, (b.n + 1) * 8);
    timing_ = cdc_timing_t{};
    timing_.bytes = b.bytes;
    timing_.candidates = h.stats[p3::kStatCand];
    timing_.overflow_spans = (uint32_t)h.stats[p3::kStatOvf];
    timing_.fixup_iterations = (uint32_t)h.stats[p3::kStatRewalk];
    timing_.walk_fallback_steps = h.stats[p3::kStatOnDemand];
    timing_.path = CDC_PATH_PIPELINE;
    timing_.timed = b.timed ? 1u : 0u;
    timing_pending_ = true;
    timing_seq_ = b.seq;
    return CDC_OK;
}

bool FastEngine::small_ok(uint64_t len) const {
    // ~len / 2^pmin records expected: keep well inside the kernel's record budget
    return small_on_ && len > 0 && len <= small::kMaxBytes && (len >> small_pmin_) <= small::kRecCap * 5 / 8;
}

int FastEngine::run_small(const uint8_t *data, uint64_t len, cdc_chunk_t *d_out, size_t out_cap, uint64_t *first,
                          hipStream_t s, const HostPlacement &place, bool host_input, const SmallFeed *feed) {
    const int rc = ensure_host_staging(1, place);
    if (rc) return rc;
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
    uint64_t *h_stats = hb_[0].stats, *h_first = hb_[0].first;
    volatile uint64_t *done = h_stats + small::kWordDone;
    *done = 0;
    small_seq_ = small_seq_ % 0xFFFFFFFEull + 1;  // 1 .. 2^32 - 2 (tags: seq << 32 | count)
    const small::Feed kfeed{feed ? feed->ready_dev : nullptr, small_seq_};
    auto feed_copy = [&]() {
        const auto tc = std::chrono::steady_clock::now();
        if (small_feed_pool_) {
            // the calling thread and whichever copy-pool helpers are awake
            // claim the pieces (work stealing: never a wait for a sleeper)
            feed->pool->copy_feed(feed->dst, feed->src, len, size_t(1) << small::kFeedLog2, feed->ready, small_seq_);
        } else {
            // (A/B: the calling thread alone)
            const uint64_t piece = 1ull << small::kFeedLog2;
            for (uint64_t off = 0; off < len; off += piece) {
                std::memcpy(feed->dst + off, feed->src + off, std::min(piece, len - off));
                std::atomic_thread_fence(std::memory_order_release);  // (x86: stores stay in order)
                feed->ready[off >> small::kFeedLog2] = small_seq_;
            }
        }
        small_copy_s_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - tc).count();
    };
    if (feed && small_feed_ == 2) feed_copy();  // (A/B: the feed copy first)
    HIP_TRY(small::launch_small(data, len, fp_, d_gear_, small_ws_, d_out, out_cap, h_stats, h_first, host_input,
                                kfeed, s));
    ++small_calls_;
    if (feed && small_feed_ != 2) {
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
    timing_.candidates = h_stats[small::kWordRecords];
    timing_.overflow_spans = 0;
    timing_.fixup_iterations = 0;
    timing_.walk_fallback_steps = 0;
    if (fp_.diag & small::kDiagStamps) {
        const uint64_t *t = h_stats + small::kWordStamp0;
        std::fprintf(stderr, "small: %llu B, us from block 0's start: last block %.2f, records %.2f, links %.2f "
                             "(%llu rounds), walk %.2f, output %.2f\n",
                     (unsigned long long)len, (t[1] - t[0]) / 100.0, (t[2] - t[0]) / 100.0, (t[3] - t[0]) / 100.0,
                     (unsigned long long)t[7], (t[4] - t[0]) / 100.0, (t[5] - t[0]) / 100.0);
        std::fprintf(stderr, "  round 0 max cycles per lane: load+trunc %llu, link %llu, successor %llu; rounds end at",
                     (unsigned long long)(t[6] & 0x1FFFFF), (unsigned long long)((t[6] >> 21) & 0x1FFFFF),
                     (unsigned long long)(t[6] >> 42));
        for (int k = 0; k < 4; ++k)
            if (h_first[2 + k]) std::fprintf(stderr, " %.2f", (h_first[2 + k] - t[0]) / 100.0);
        if (feed) std::fprintf(stderr, "; block 0 fed at %.2f; host copy %.2f us", (h_first[6] - t[0]) / 100.0,
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
    small_last_len_ = 0;
    if (h_stats[small::kWordFallback]) {
        ++small_fallbacks_;
        return kSmallFallback;
    }
    first[0] = 0;
    first[1] = h_first[1];
    small_last_len_ = len;
    small_last_staged_ = host_input;
    small_last_stream_ = s;
    return CDC_OK;
}

// Batch events: [0] before its scan launch, [1] after it (before the
// resolve), [2] after the resolve.
const cdc_timing_t &FastEngine::timing() {
    if (timing_pending_) {
        timing_pending_ = false;
        (void)timing_back((uint32_t)(seq_ - 1 - timing_seq_), timing_);
    }
    return timing_;
}

int FastEngine::timing_back(uint32_t back, cdc_timing_t &out) {
    if (back >= kTimeRing || back >= seq_) {
        set_error("cdc_debug_timing_back: no such FastCDC batch in the event ring");
        return CDC_EINVAL;
    }
    if (&out != &timing_) out = timing_;
    hipEvent_t *ev = tev_[(seq_ - 1 - back) % kTimeRing];
    float t01 = 0, t12 = 0, t02 = 0;
    HIP_TRY(hipSetDevice(device_));
    out.path = CDC_PATH_PIPELINE;
    out.timed = tev_timed_[(seq_ - 1 - back) % kTimeRing] ? 1u : 0u;
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

int64_t FastEngine::debug_copy(int what, void *out, size_t max_bytes) {
    if (what >= 2 && what <= 7) {  // the small kernel's scratch, as the last call left it
        const bool whole = what >= 5;  // 5..7: the arrays of 2..4 at their full size
        const int arr = whole ? what - 3 : what;
        if (small_last_len_ == 0 || (arr == 4 && !small_last_staged_)) {
            set_error(small_last_len_ ? "debug_copy: the last one-launch call read device input (no copy)"
                                      : "debug_copy: the last FastCDC call was not a one-launch call");
            return CDC_EINVAL;
        }
        const uint64_t blocks =
            whole ? small::kMaxBlocks : (small_last_len_ + small::kBlockBytes - 1) / small::kBlockBytes;
        const void *src = arr == 2 ? (const void *)small_ws_.bcnt
                          : arr == 3 ? (const void *)small_ws_.brec
                                     : (const void *)small_ws_.copy;
        size_t bytes = arr == 2 ? blocks * 4
                       : arr == 3 ? blocks * small::kBlockRecCap * 8
                                  : (size_t)(whole ? small::kMaxBytes : small_last_len_);
        if (bytes > max_bytes) bytes = max_bytes;
        HIP_TRY(hipSetDevice(device_));
        HIP_TRY(hipStreamSynchronize(small_last_stream_));
        if (bytes) HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
        return (int64_t)bytes;
    }
    if (seq_ == 0) {
        set_error("debug_copy: no FastCDC batch yet");
        return CDC_EINVAL;
    }
    const FastBatch &last = fb_[(seq_ - 1) % 3];
    const Candidates &cand = fs_[last.slot].cand;
    const void *src = nullptr;
    size_t bytes = 0;
    if (what == 0) {
        src = cand.count;
        bytes = last.spans * 4;
    } else if (what == 1) {
        src = cand.pos;
        bytes = last.spans * cap_ * 4;
    } else {
        set_error("debug_copy: unknown array");
        return CDC_EINVAL;
    }
    if (bytes > max_bytes) bytes = max_bytes;
    HIP_TRY(hipSetDevice(device_));
    if (bytes) HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return (int64_t)bytes;
}

}  // namespace cdc
