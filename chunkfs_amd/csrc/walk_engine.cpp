// walk_engine.cpp -- host orchestration of the segment-walk engine (walk.hip;
// DESIGN.md "Segment walk", "Async walk batches").
//
// Per batch: the stream tables (zero-copy, or uploaded when they changed) ->
// bitmap pass -> walk -> fix-up rounds in groups, the output queued behind the
// first group -> one host wait in the common case.
#include "walk_engine.hpp"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>

namespace cdc {

namespace {
// GF(2) remainder modulo the Rabin polynomial (host-side table build).
uint64_t gf2_mod(uint64_t x, uint64_t p) {
    const int dp = 63 - __builtin_clzll(p);
    while (x) {
        const int dx = 63 - __builtin_clzll(x);
        if (dx < dp) break;
        x ^= p << (dx - dp);
    }
    return x;
}

uint64_t splitmix_word(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
}  // namespace

int WalkEngine::validate(cdc_algo_t algo, uint32_t min, uint32_t avg, uint32_t max, WalkConfig &cfg,
                         std::string &describe) {
    // Size rules (oracle_cdc_check): 0 < min <= avg <= max, and the
    // bytes each rule reads before the first tested position.
    if (min == 0 || min > avg || avg > max || (algo == CDC_ALGO_ULTRA && min < 8) ||
        (algo == CDC_ALGO_LEAP && min < 32) || (algo == CDC_ALGO_RABIN && avg < 2)) {
        set_error("invalid sizes: need 0 < min <= avg <= max (UltraCDC min >= 8, LeapCDC min >= 32, RabinCDC avg >= 2)");
        return CDC_EINVAL;
    }
    if (algo == CDC_ALGO_SEQ &&
        (cfg.seq_mode > 1 || cfg.seq_length == 0 || cfg.seq_jump_trigger == 0 || cfg.seq_jump_size == 0)) {
        set_error("invalid SeqCDC config: mode 0/1, seq_length > 0, jump_trigger > 0, jump_size > 0");
        return CDC_EINVAL;
    }
    if (algo == CDC_ALGO_AE) {  // window 0: the default for avg
        if (cfg.ae_window == 0) cfg.ae_window = cdc_ae_default_window(avg);
        if (cfg.ae_mode > 1 || (uint64_t)cfg.ae_window + 1 > max) {
            set_error("invalid AE config: mode 0 (Max) / 1 (Min), 1 <= window and window + 1 <= max");
            return CDC_EINVAL;
        }
    }
    const char *name = algo == CDC_ALGO_RABIN ? "RabinCDC" : algo == CDC_ALGO_ULTRA ? "UltraCDC"
                     : algo == CDC_ALGO_LEAP ? "LeapCDC" : algo == CDC_ALGO_AE ? "AE" : "SeqCDC";
    char buf[256];
    // impl Debug (rabin.rs:28-32, ultra.rs:24-28, leap.rs:24-28, seq.rs:34-38)
    if (algo == CDC_ALGO_AE)
        std::snprintf(buf, sizeof buf,
                      "%s, sizes: SizeParams { min: %u, avg: %u, max: %u }, window: %u, mode: %s [MI355X gfx950]", name,
                      min, avg, max, cfg.ae_window, cfg.ae_mode ? "Min" : "Max");
    else if (algo == CDC_ALGO_SEQ)
        std::snprintf(buf, sizeof buf, "%s, sizes: SizeParams { min: %u, avg: %u, max: %u }, mode: %s [MI355X gfx950]",
                      name, min, avg, max, cfg.seq_mode ? "Decreasing" : "Increasing");
    else
        std::snprintf(buf, sizeof buf, "%s, sizes: SizeParams { min: %u, avg: %u, max: %u } [MI355X gfx950]", name,
                      min, avg, max);
    describe = buf;
    return CDC_OK;
}

int WalkEngine::create(cdc_algo_t algo, uint32_t min, uint32_t avg, uint32_t max, const WalkConfig &cfg, int device,
                       std::unique_ptr<WalkEngine> &out) {
    std::unique_ptr<WalkEngine> w(new WalkEngine());
    w->algo_ = algo;
    w->min_ = min;
    w->avg_ = avg;
    w->max_ = max;
    w->cfg_ = cfg;
    w->device_ = device;
    if (const char *v = std::getenv("CHUNKFS_AMD_WALK_ASYNC")) w->async_ = std::atoi(v) != 0;
    if (const char *v = std::getenv("CHUNKFS_AMD_WALK_CTX")) w->n_ctx_ = std::max(2, std::min(kCtxMax, std::atoi(v)));
    const int rc = w->init();
    if (rc != CDC_OK) return rc;
    out = std::move(w);
    return CDC_OK;
}

int WalkEngine::init() {
    walk::WalkParams &wp = wp_;
    wp.algo = (uint32_t)algo_;
    wp.min = min_;
    wp.avg = avg_;
    wp.max = max_;
    wp.rabin_mask = (1ull << cdc_log2_round(avg_)) - 1;

    const uint64_t lspan = avg_ > min_ ? (uint64_t)(avg_ - min_) : 1;
    const uint32_t lb = cdc_log2_round(lspan);
    wp.leap_thr = CDC_LEAP_THRESHOLD[lb > 32 ? 32 : lb];
    wp.seq_mode = cfg_.seq_mode;
    wp.seq_len = cfg_.seq_length;
    wp.seq_trig = cfg_.seq_jump_trigger;
    wp.seq_jump = cfg_.seq_jump_size;
    wp.ae_mode = cfg_.ae_mode;  // (validate resolved the default window)
    wp.ae_window = cfg_.ae_window;
    // Segments of 2^seg_log2 bytes (one lane each) and a warm-up of `warm`
    // bytes; CHUNKFS_AMD_WALK="seg_log2,warm_over_avg" overrides (experiments).
    // Defaults (tools/walk_bench.py sweeps on MI355X): segments of
    // 32 KiB whatever the average (at avg 64 KiB, 32 KiB segments beat 256 KiB
    // ones for every rule: more lanes, a shorter walk per lane and cheaper
    // fix-up re-walks; profiles/r02ak_walk_avg64k_segments.log), a warm-up of
    // 8 avg (a chain from an arbitrary start merges with the true one within a
    // few content-defined cuts).
    // Bitmap mode: Rabin when every tested digest is a full
    // window (min >= 48), UltraCDC, LeapCDC, and SeqCDC when its run length
    // fits a 64-bit step (seq_length <= 63).  CHUNKFS_AMD_WALK_BYTES=1 forces
    // the byte walks (A/B experiments).
    // AE has no byte walk: always its R bitmap, CHUNKFS_AMD_WALK_BYTES or not.
    wp.nbm = algo_ == CDC_ALGO_RABIN ? (min_ >= CDC_RABIN_WINDOW ? 1u : 0u)
           : algo_ == CDC_ALGO_ULTRA ? 3u : algo_ == CDC_ALGO_LEAP ? 2u
           : algo_ == CDC_ALGO_AE ? 1u : (wp.seq_len <= 63 ? 1u : 0u);
    if (const char *b = std::getenv("CHUNKFS_AMD_WALK_BYTES"))
        if (std::atoi(b) != 0 && algo_ != CDC_ALGO_AE) wp.nbm = 0;
    // Bitmap mode walks with a wave per segment (walk.hip wwalk_kernel), byte
    // mode with a lane per segment (walk_kernel).
    // Lane walks: 32 KiB segments whatever the average (profiles/r02ak).
    // Wave walks: 128 KiB (Rabin, Leap) / 256 KiB segments, 8 avg warm-up
    // (profiles/r03_walk/r03w_walk_seg_sweep.txt: a wave walks thousands of
    // positions per step, so fewer, longer segments cut the warm-up share).
    // Warm-up, in averages: chains from an arbitrary start merge within a few
    // content-defined cuts.  Lane walks: 8 avg, SeqCDC 16
    // (profiles/r02ag_walk_warm_sweep.log).  Wave walks: Rabin 8, UltraCDC and
    // SeqCDC 16, LeapCDC 24 (its chains merge slowest; the fix-up rounds a
    // shorter warm-up leaves cost more than the walk it saves,
    // profiles/r03_walk/r03ab_walk_warm_ahead_sweep.txt).
    uint64_t warm_mult = !wp.nbm ? (algo_ == CDC_ALGO_SEQ ? 16 : 8)
                       : algo_ == CDC_ALGO_RABIN ? 8 : algo_ == CDC_ALGO_LEAP ? 24 : 16;
    // Segments: lane walks 32 KiB whatever the average (profiles/r02ak).  Wave
    // walks: at least 128 KiB (Rabin) / 256 KiB and at least the warm-up, so
    // that the warm-up stays a fraction of each wave's walk (a wave walks
    // thousands of positions per step; r03w_walk_seg_sweep.txt), up to 4 MiB.
    seg_log2_ = !wp.nbm ? 15 : algo_ == CDC_ALGO_RABIN ? 17 : 18;
    if (wp.nbm) {
        const uint32_t wl = ceil_log2(warm_mult * avg_);
        if (wl > seg_log2_) seg_log2_ = wl < 22 ? wl : 22;
    }
    // The per-segment start list holds segment/min + 2 entries: keep it <= ~4k
    // (tiny min), and segments >= 4 KiB.
    const uint32_t lmin = 63 - (uint32_t)__builtin_clzll((uint64_t)min_) + 12;
    if (seg_log2_ > lmin) seg_log2_ = lmin < 12 ? 12 : lmin;
    if (const char *w = std::getenv("CHUNKFS_AMD_WALK")) {
        unsigned a = 0, b = 0;
        if (std::sscanf(w, "%u,%u", &a, &b) == 2 && a >= 10 && a <= 30) {
            seg_log2_ = a;
            warm_mult = b;
        }
    }
    if (algo_ == CDC_ALGO_AE && seg_log2_ < 12) seg_log2_ = 12;  // its bitmap pass steps 4 KiB at a time
    wp.warm = warm_mult * avg_;
    // CHUNKFS_AMD_AHEAD="after,max" overrides the run-ahead schedule (experiments).
    if (const char *a = std::getenv("CHUNKFS_AMD_AHEAD")) {
        unsigned x = 0, y = 0;
        if (std::sscanf(a, "%u,%u", &x, &y) == 2 && y >= 1) {
            ahead_after_ = x;
            ahead_max_ = y;
        }
    }
    wp.ahead = 1;
    wp.bits_fine = 1;
    if (const char *f = std::getenv("CHUNKFS_AMD_BITS_FINE")) wp.bits_fine = std::atoi(f) != 0 ? 1u : 0u;
    if (const char *f = std::getenv("CHUNKFS_AMD_WALK_FUSED")) fused_ = std::atoi(f) != 0;
    wp.cap = (uint32_t)((1ull << seg_log2_) / min_ + 2);
    wp.seg_words = (uint32_t)((1ull << seg_log2_) / 64);
    wp.piece_log2 = seg_log2_ < 15 ? seg_log2_ : 15;  // data-parallel passes: 32 KiB pieces
    wp.bm = nullptr;
    for (auto &ev : ev_) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipMalloc(&d_tabs_, 768 * sizeof(uint64_t)));
    wp.tabs = d_tabs_;
    return load_tables(rabin_poly_);
}

WalkEngine::~WalkEngine() {
    for (auto &c : ctx_) c.reset();  // (each completes the batch it has in hand)
    (void)hipFree(d_tabs_);
    (void)hipFree(ws_);
    (void)hipHostFree(h_block_);
    for (auto &ev : ev_)
        if (ev) (void)hipEventDestroy(ev);
}

// Tables: Rabin mod/out of polynomial P (appending a byte; sliding one out of
// the window), LeapCDC window-hash table; and the digest's top-byte shift.
int WalkEngine::load_tables(uint64_t P) {
    uint64_t t[768];
    const int deg = 63 - __builtin_clzll(P);
    for (uint64_t b = 0; b < 256; ++b) {
        t[b] = gf2_mod(b << deg, P) | (b << deg);
        uint64_t h = b;
        for (uint32_t i = 1; i < CDC_RABIN_WINDOW; ++i) h = gf2_mod(h << 8, P);
        t[256 + b] = h;
        t[512 + b] = splitmix_word(CDC_LEAP_SEED + (b + 1) * 0x9E3779B97F4A7C15ull);
    }
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipMemcpy(d_tabs_, t, sizeof t, hipMemcpyHostToDevice));
    wp_.rabin_shift = (uint32_t)deg - 8;
    return CDC_OK;
}

int WalkEngine::set_rabin_poly(uint64_t P) {
    rabin_poly_ = P;
    for (auto &c : ctx_) c.reset();  // (the contexts are made again, with this polynomial)
    // The degree decides the bitmap kernel and whether it writes the quiet-run
    // summary (walk::bits_write_summary): the workspace is laid out again.
    (void)hipFree(ws_);
    ws_ = nullptr;
    ws_segs_ = 0;
    ws_streams_ = 0;
    return load_tables(P);
}

int WalkEngine::ensure_host_block(size_t n, const HostPlacement &place) {
    if (h_block_ && h_streams_ >= n) return CDC_OK;
    (void)hipHostFree(h_block_);
    h_block_ = nullptr;
    h_streams_ = 0;
    const size_t W = align_up(n + 64, 8);  // words per table (each starts a 64-byte line)
    const size_t words = 4 * W + 4 + 4 * walk::kMaxFixRounds;
    HIP_TRY(place.host_malloc(&h_block_, words * sizeof(uint64_t), hipHostMallocCoherent));
    h_streams_ = W - 1;
    uint64_t *h = static_cast<uint64_t *>(h_block_);
    tab_.h_ptrs = h;
    tab_.h_lens = h + W;
    tab_.h_sb = h + 2 * W;  // [n+1]
    h_first_ = h + 3 * W;   // [n+1]
    h_flags_ = h + 4 * W;   // flags[4] ++ the round blocks
    return CDC_OK;
}

int WalkEngine::ensure_workspace(uint64_t segs, size_t n) {
    if (ws_ && segs <= ws_segs_ && n <= ws_streams_) return CDC_OK;
    const uint64_t S = segs > ws_segs_ ? segs + segs / 4 + 16 : ws_segs_;
    const size_t N = n > ws_streams_ ? n + 64 : ws_streams_;
    const uint64_t nb = S / walk::kScanBlock + 2;
    const size_t A = 256;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, A);
        return o;
    };
    const size_t oE = take(S * 8), oX = take(S * 8), oXs = take(S * 8), oEs = take(S * 8), oP = take((S + 1) * 8);
    const size_t oN = take(S * 4), oL = take(S * (size_t)wp_.cap * 8), oB = take((nb + 1) * 8);
    const size_t oF = take((N + 1) * 8), oG = take((4 + 4 * walk::kMaxFixRounds) * 8), oGo = take(16);
    const size_t oBM = take(S * (size_t)wp_.seg_words * wp_.nbm * 8);  // predicate bitmaps
    const bool jt = algo_ == CDC_ALGO_LEAP && wp_.nbm;
    const size_t oJT = take(jt ? S * (size_t)wp_.seg_words * 24 : 0);  // LeapCDC word tables
    const size_t oJ8 = take(jt ? S * (size_t)wp_.seg_words * 6 : 0);   // and 512-position block tables
    bool rsum = walk::bits_write_summary(wp_);  // quiet runs (CHUNKFS_AMD_QUIET=0: off, A/B)
    if (const char *q = std::getenv("CHUNKFS_AMD_QUIET")) rsum = rsum && std::atoi(q) != 0;
    const size_t oRS = take(rsum ? S * (size_t)wp_.seg_words / 8 * (algo_ == CDC_ALGO_RABIN ? 2 : 1) : 0);  // quiet-run summary
    const size_t oQS = take(rsum ? S : 0);  // and per segment
    const bool ae = algo_ == CDC_ALGO_AE;  // AE: per-word and per-64-word maxima
    const size_t oM64 = take(ae ? S * (size_t)wp_.seg_words * 4 : 0);
    const size_t oM4k = take(ae ? S * (size_t)wp_.seg_words / 64 * 4 : 0);
    const size_t o_ptrs = take(N * 8), o_lens = take(N * 8), o_sb = take((N + 1) * 8);
    (void)hipFree(ws_);
    ws_ = nullptr;
    ws_segs_ = 0;
    ws_streams_ = 0;
    HIP_TRY(hipMalloc(&ws_, off));
    ++ws_gen_;  // the stream tables move: re-upload them
    ws_segs_ = S;
    ws_streams_ = N;
    char *b = static_cast<char *>(ws_);
    st_.E = reinterpret_cast<uint64_t *>(b + oE);
    st_.X = reinterpret_cast<uint64_t *>(b + oX);
    st_.Xs = reinterpret_cast<uint64_t *>(b + oXs);
    st_.Es = reinterpret_cast<uint64_t *>(b + oEs);
    st_.P = reinterpret_cast<uint64_t *>(b + oP);
    st_.N = reinterpret_cast<uint32_t *>(b + oN);
    st_.list = reinterpret_cast<uint64_t *>(b + oL);
    st_.bsum = reinterpret_cast<uint64_t *>(b + oB);
    st_.first = reinterpret_cast<uint64_t *>(b + oF);
    st_.flags = reinterpret_cast<unsigned long long *>(b + oG);
    go_ = reinterpret_cast<uint64_t *>(b + oGo);
    flags_clean_ = false;  // (fresh memory: the next call initialises the flag blocks)
    wp_.bm = wp_.nbm ? reinterpret_cast<uint64_t *>(b + oBM) : nullptr;
    wp_.jt = jt ? reinterpret_cast<uint8_t *>(b + oJT) : nullptr;
    wp_.jt8 = jt ? reinterpret_cast<uint16_t *>(b + oJ8) : nullptr;
    wp_.rsum = rsum ? reinterpret_cast<uint64_t *>(b + oRS) : nullptr;
    wp_.qseg = rsum ? reinterpret_cast<uint8_t *>(b + oQS) : nullptr;
    wp_.ae_m64 = ae ? reinterpret_cast<uint32_t *>(b + oM64) : nullptr;
    wp_.ae_m4k = ae ? reinterpret_cast<uint32_t *>(b + oM4k) : nullptr;
    tab_.d_ptrs = reinterpret_cast<const uint8_t **>(b + o_ptrs);
    tab_.d_lens = reinterpret_cast<uint64_t *>(b + o_lens);
    tab_.d_sb = reinterpret_cast<uint64_t *>(b + o_sb);
    return CDC_OK;
}

int64_t WalkEngine::chunk_batch(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                                size_t out_cap, uint64_t *first, hipStream_t s, const HostPlacement &place) {
    timing_ = cdc_timing_t{};
    timing_.path = CDC_PATH_EMPTY;
    last_segs_ = 0;
    last_end_ = 0;
    for (size_t i = 0; i < n; ++i) timing_.bytes += lens[i];
    if (n == 0) {
        if (first) first[0] = 0;
        return 0;
    }
    int rc = ensure_host_block(n, place);
    if (rc) return rc;
    const uint64_t segs = tab_.fill(n, d_streams, lens, seg_log2_);
    if (segs == 0) {  // every stream is empty
        for (size_t i = 0; i <= n; ++i) first[i] = 0;
        return 0;
    }
    last_segs_ = segs;
    rc = ensure_workspace(segs, n);
    if (rc) return rc;
    StreamTable st;
    rc = tab_.publish(n, timing_.bytes, seg_log2_, segs, ws_gen_, s, st);
    if (rc) return rc;
    rc = run(st, d_out, out_cap, n, first, s);
    if (rc) return rc;
    return (int64_t)first[n];
}

int WalkEngine::run(const StreamTable &st, cdc_chunk_t *d_out, uint64_t out_cap, size_t n, uint64_t *first,
                    hipStream_t s) {
    uint64_t *h_first = h_first_, *h_flags = h_flags_;
    uint64_t *h_rf = h_flags + 4;
    const uint32_t R = max_rounds_ < walk::kMaxFixRounds ? max_rounds_ : walk::kMaxFixRounds;
    HIP_TRY(hipEventRecord(ev_[0], s));
    // (the previous call's end kernel resets the flag blocks when it ends
    // the call: then no init launch here)
    if (!flags_clean_) HIP_TRY(walk::launch_flags_init(st_.flags, R, s));
    flags_clean_ = false;
    static const bool diag = std::getenv("CHUNKFS_AMD_WALKDIAG") != nullptr;  // phase times
    auto lap = [&](const char *what) -> int {
        if (!diag) return CDC_OK;
        static auto t_last = std::chrono::steady_clock::now();
        HIP_TRY(hipStreamSynchronize(s));
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "  walkdiag %-6s %9.3f ms\n", what,
                     std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
        return CDC_OK;
    };
    (void)lap("start");
    HIP_TRY(walk::launch_bits(st, wp_, s));
    (void)lap("bits");
    HIP_TRY(walk::launch_walk(st, wp_, st_, s));
    (void)lap("walk");
    HIP_TRY(hipEventRecord(ev_[1], s));
    // Jacobi rounds: re-walk every segment whose entry is not its predecessor's
    // exit, until none is.  Rounds are launched in groups without a host sync:
    // round r counts into its own flag block (rf + 4 r) and returns at once on
    // the device when round r-1 changed no exit (WalkState::gate), so the host
    // waits once per group instead of once per round.
    // The output is queued right behind the first group, gated on the device
    // by the same rule (walk::launch_emit's egate): when that group settles
    // -- the common case -- the call needs one host wait, not two.
    // The first group is one round: on random data the first round settles
    // every segment (its re-walks meet the old chains), and the gated no-op
    // rounds after it cost ~14 us each (snapshot + fix launches).
    constexpr uint32_t kGroup = 4;
    unsigned long long *rf = st_.flags + 4;
    uint64_t rewalked = 0, round_errors = 0;
    bool settled = false, quiet_stop = false, queued = false, fused = false;
    uint32_t launched = 0, last_round = 0;
    while (launched < R && !settled) {
        const uint32_t grp = launched == 0 ? walk::kFirstGroupRounds : kGroup;
        const uint32_t end = launched + grp < R ? launched + grp : R;
        for (uint32_t r = launched; r < end; ++r) {
            // Plain Jacobi for the first ahead_after_ rounds, then run-ahead
            // re-walks (walk.hip fix_kernel) so long non-merging stretches
            // settle before the serial pass would be needed.
            wp_.ahead = r < ahead_after_ ? 1u : ahead_max_;
            walk::WalkState ws = st_;
            ws.flags = rf + 4 * r;
            ws.gate = r ? rf + 4 * (r - 1) : nullptr;
            const auto t0 = std::chrono::steady_clock::now();
            HIP_TRY(walk::launch_fix(st, wp_, ws, s, r != 0));  // (round 0's snapshot: written by the walk)
            if (diag) {
                HIP_TRY(hipStreamSynchronize(s));
                std::fprintf(stderr, "  walkdiag round %u %.3f ms\n", r,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
        }
        queued = launched == 0 && !diag;
        launched = end;
        // Fused end (walk::launch_finish_emit): the prefix, first[] and the
        // flag blocks go straight into the pinned host block -- no D2H
        // copies -- and the flags are reset for the next call when it ends
        // this one.
        fused = queued && fused_ && walk::finish_fits(st);
        if (fused) {
            HIP_TRY(walk::launch_finish_emit(st, wp_, st_, d_out, out_cap, s, rf, launched, launched, go_, h_first,
                                             h_flags));
        } else {
            if (queued) {
                HIP_TRY(walk::launch_emit(st, wp_, st_, d_out, out_cap, s, rf, launched));
                HIP_TRY(hipMemcpyAsync(h_first, st_.first, (n + 1) * 8, hipMemcpyDeviceToHost, s));
            }
            HIP_TRY(hipMemcpyAsync(h_flags, st_.flags, (4 + (size_t)launched * 4) * 8, hipMemcpyDeviceToHost, s));
        }
        if (queued) HIP_TRY(hipEventRecord(ev_[2], s));
        HIP_TRY(hipStreamSynchronize(s));
        // The first round that settled everything, or whose changed exits
        // were mostly quiet-run re-walks (zero-filled / constant regions:
        // chains there keep their phase, so each round moves the true one a
        // single segment; the in-order pass takes such a region in one go).
        // Later rounds of the group returned at once on the device (the same
        // rule, walk.hip round_stops).
        for (uint32_t r = 0; r < launched; ++r) {
            const int v = walk::round_verdict(h_rf[4 * r], h_rf[4 * r + 3] >> 32);  // (walk.hpp: shared rule)
            if (v == walk::kRoundSettled) {
                settled = true;
                break;
            }
            if (v == walk::kRoundQuiet) {
                last_round = r;
                quiet_stop = true;
                break;
            }
        }
        if (quiet_stop) break;
    }
    for (uint32_t r = 0; r < launched; ++r) {
        round_errors += h_rf[4 * r + 1];
        rewalked += h_rf[4 * r + 3] & 0xFFFFFFFFull;
    }
    if (diag) {
        std::fprintf(stderr, "  walkdiag rounds %u settled %d:", launched, (int)settled);
        for (uint32_t r = 0; r < launched && r < 24; ++r)
            std::fprintf(stderr, " %llu/%llu", (unsigned long long)h_rf[4 * r + 3], (unsigned long long)h_rf[4 * r]);
        std::fprintf(stderr, "\n");
    }
    // Chains that never merge (periodic data): one exact in-order pass from
    // the lowest segment the last round changed.
    if (!settled) {
        const uint32_t lr = quiet_stop ? last_round : launched - 1;  // the last round that ran
        HIP_TRY(hipMemcpyAsync(st_.flags + 2, rf + 4 * lr + 2, 8, hipMemcpyDeviceToDevice, s));
        HIP_TRY(walk::launch_serial(st, wp_, st_, s));
    }
    (void)lap("fixup");
    // The gated output queued after the first group ran on the device exactly
    // when that group settled by the same rule (emit_skips), i.e. when the
    // loop stopped after it: launched == kFirstGroupRounds.
    const bool gated_ran = queued && settled && launched == walk::kFirstGroupRounds;
    flags_clean_ = gated_ran && fused;  // (finish_kernel reset them)
    last_end_ = gated_ran ? (fused ? 0u : 1u) : 2u;
    if (!gated_ran) {  // (else the gated output already ran)
        HIP_TRY(walk::launch_emit(st, wp_, st_, d_out, out_cap, s));
        HIP_TRY(hipMemcpyAsync(h_flags, st_.flags, 4 * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h_first, st_.first, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(ev_[2], s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (h_flags[1] + round_errors != 0) {
        set_error("segment walk: chunk list or output bound exceeded (internal error)");
        return CDC_EDEVICE;
    }
    std::memcpy(first, h_first, (n + 1) * 8);
    float t01 = 0, t12 = 0, t02 = 0;
    HIP_TRY(hipEventElapsedTime(&t01, ev_[0], ev_[1]));
    HIP_TRY(hipEventElapsedTime(&t12, ev_[1], ev_[2]));
    HIP_TRY(hipEventElapsedTime(&t02, ev_[0], ev_[2]));
    timing_.scan_ms = t01;
    timing_.resolve_ms = t12;
    timing_.total_ms = t02;
    timing_.fixup_iterations = (uint32_t)rewalked;
    timing_.overflow_spans = settled ? 0u : 1u;
    timing_.path = CDC_PATH_WALK;
    timing_.timed = 1;
    return CDC_OK;
}

int WalkEngine::debug_params(uint64_t *v, size_t n) const {
    const uint64_t w[kDebugWords] = {wp_.nbm, seg_log2_, wp_.warm, wp_.cap, wp_.piece_log2,
                                     wp_.rabin_mask, wp_.leap_thr, last_segs_, last_end_};
    for (size_t i = 0; i < n && i < (size_t)kDebugWords; ++i) v[i] = w[i];
    return kDebugWords;
}

// ---- async batches ---------------------------------------------------------

// A context, its stream and the host thread that runs its batches.
struct WalkEngine::Worker {
    std::unique_ptr<WalkEngine> ctx;  // the handle's configuration, never async itself
    hipStream_t stream = nullptr;
    int device = 0;
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    bool has_job = false, stop = false;
    bool done = true;    // no batch posted or running
    bool fresh = false;  // ran a batch since the last drain
    uint64_t seq = 0;    // that batch's number
    std::vector<const uint8_t *> ptrs;
    std::vector<uint64_t> lens;
    cdc_chunk_t *out = nullptr;
    size_t cap = 0;
    uint64_t *first = nullptr;
    const HostPlacement *place = nullptr;  // the handle's (it outlives the batch: a drain comes first)
    hipEvent_t after = nullptr;  // recorded on the caller's stream at submit: the batch's input is complete there
    int64_t rc = 0;
    std::string err;

    void loop() {
        (void)hipSetDevice(device);
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv.wait(lk, [&] { return stop || has_job; });
            if (has_job) {  // (a stop request waits for the batch in hand)
                has_job = false;
                lk.unlock();
                // the context's stream runs nothing of this batch before the
                // caller's stream reached the submit
                int64_t r = CDC_OK;
                if (hipStreamWaitEvent(stream, after, 0) != hipSuccess) {
                    set_error("walk batch: hipStreamWaitEvent on the caller's stream failed");
                    r = CDC_EDEVICE;
                }
                if (r == CDC_OK)
                    r = ctx->chunk_batch(ptrs.size(), ptrs.data(), lens.data(), out, cap, first, stream, *place);
                std::string e = r < 0 ? std::string(last_error()) : std::string();
                lk.lock();
                rc = r;
                err = std::move(e);
                done = true;
                cv.notify_all();
                continue;
            }
            return;
        }
    }
    void wait_done(std::unique_lock<std::mutex> &lk) {
        cv.wait(lk, [&] { return done; });
    }
    ~Worker() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
        if (stream) (void)hipStreamSynchronize(stream);
        ctx.reset();
        if (after) (void)hipEventDestroy(after);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// Batch k goes to context k % n_ctx_ (2 by default), once that context's
// previous batch is done; a failure of that batch fails this call (after the
// other contexts are drained), as FastCDC's collection does.
int64_t WalkEngine::submit(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                           size_t out_cap, uint64_t *first, hipStream_t s, const HostPlacement &place) {
    const int c = (int)(seq_ % (uint64_t)n_ctx_);
    if (!ctx_[c]) {
        std::unique_ptr<Worker> w(new Worker());
        int rc = create(algo_, min_, avg_, max_, cfg_, device_, w->ctx);
        if (rc) return rc;
        w->ctx->async_ = false;
        if (rabin_poly_ != CDC_RABIN_POLY) rc = w->ctx->set_rabin_poly(rabin_poly_);
        if (rc) return rc;
        w->device = device_;
        HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&w->after, hipEventDisableTiming));
        Worker *wp = w.get();
        w->th = std::thread([wp] { wp->loop(); });
        ctx_[c] = std::move(w);
    }
    Worker &w = *ctx_[c];
    {
        std::unique_lock<std::mutex> lk(w.m);
        w.wait_done(lk);
        if (w.fresh && w.rc < 0) {
            const int64_t rc = w.rc;
            const std::string msg = w.err;
            lk.unlock();
            (void)drain();
            set_error(msg);
            return rc;
        }
        // (the context's previous batch is done: its wait on this event is long past)
        HIP_TRY(hipEventRecord(w.after, s));
        w.ptrs.assign(d_streams, d_streams + n);
        w.lens.assign(lens, lens + n);
        w.out = d_out;
        w.cap = out_cap;
        w.first = first;
        w.place = &place;
        w.seq = seq_;
        w.rc = 0;
        w.err.clear();
        w.done = false;
        w.fresh = true;
        w.has_job = true;
    }
    w.cv.notify_all();
    ++seq_;
    in_flight_ = true;
    return 0;
}

int64_t WalkEngine::drain() {
    int64_t res = 0, err = 0;
    std::string msg;
    uint64_t last = 0;
    bool any = false;
    for (auto &wp : ctx_) {
        if (!wp) continue;
        Worker &w = *wp;
        std::unique_lock<std::mutex> lk(w.m);
        w.wait_done(lk);
        if (!w.fresh) continue;
        w.fresh = false;
        if (w.rc < 0 && !err) {
            err = w.rc;
            msg = w.err;
        }
        if (!any || w.seq > last) {
            any = true;
            last = w.seq;
            res = w.rc;
            timing_ = w.ctx->timing_;
        }
    }
    in_flight_ = false;
    if (err) {
        set_error(msg);
        return err;
    }
    return res;
}

}  // namespace cdc
