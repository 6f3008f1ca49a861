// engine.cpp -- the handle behind the C ABI: argument checks, dispatch of the
// device batches to the handle's backend (FastEngine, WalkEngine or the
// fixed-size launch below), the drain results held for cdc_batch_sync, the
// hash calls (HashEngine) and the debug entries.  The host boundary is the
// handle's HostPath (host_path.hpp, hostpath.cpp).
#include "engine.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fast_engine.hpp"
#include "hash_engine.hpp"
#include "host_path.hpp"
#include "walk_engine.hpp"

namespace cdc {

namespace {
thread_local std::string g_last_error;
}  // namespace

void set_error(const std::string &msg) { g_last_error = msg; }
const char *last_error() { return g_last_error.c_str(); }

int Engine::create(cdc_algo_t algo, uint32_t min, uint32_t avg, uint32_t max,
                   int device, Engine **out) {
    WalkConfig cfg;  // (the rule's defaults)
    return create_handle(algo, cfg, min, avg, max, device, out);
}

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
    return create_handle(CDC_ALGO_SEQ, cfg, min, avg, max, device, out);
}

int Engine::create_ae(uint32_t mode, uint32_t window, uint32_t min, uint32_t avg, uint32_t max, int device,
                      Engine **out) {
    WalkConfig cfg;
    cfg.ae_mode = mode;
    cfg.ae_window = window;
    return create_handle(CDC_ALGO_AE, cfg, min, avg, max, device, out);
}

// Validation (before any HIP call), the handle, then its backend.
int Engine::create_handle(cdc_algo_t algo, WalkConfig &cfg, uint32_t min, uint32_t avg, uint32_t max, int device,
                          Engine **out) {
    if (!out) {
        set_error("cdc_create: out is NULL");
        return CDC_EINVAL;
    }
    *out = nullptr;
    const bool walk = algo == CDC_ALGO_RABIN || algo == CDC_ALGO_ULTRA || algo == CDC_ALGO_LEAP ||
                      algo == CDC_ALGO_SEQ || algo == CDC_ALGO_AE;
    std::string describe;
    int rc = CDC_OK;
    if (walk) {
        rc = WalkEngine::validate(algo, min, avg, max, cfg, describe);
    } else if (algo == CDC_ALGO_FASTCDC) {
        rc = FastEngine::validate(min, avg, max, describe);
    } else if (algo == CDC_ALGO_FIXED) {
        if (min == 0) {
            set_error("FSChunker chunk size must be > 0");
            return CDC_EINVAL;
        }
        char buf[128];
        std::snprintf(buf, sizeof buf, "Fixed size chunking, chunk size: %u [MI355X gfx950]", min);
        describe = buf;
    } else {
        set_error("SuperCDC is not implemented on MI355X: its chunk records (supercdc.rs:10, 37-50) "
                  "follow cdc-chunkers 0.1.3, absent offline (SURVEY.md §8c)");
        return CDC_ENOTSUP;
    }
    if (rc != CDC_OK) return rc;
    Engine *e = new Engine();
    e->algo_ = algo;
    e->min_ = min;
    e->avg_ = avg;
    e->max_ = max;
    e->device_ = device;
    e->describe_ = describe;
    rc = e->init();
    if (rc == CDC_OK && walk) rc = WalkEngine::create(algo, min, avg, max, cfg, device, e->walk_);
    if (rc == CDC_OK && algo == CDC_ALGO_FASTCDC) rc = FastEngine::create(min, avg, max, device, e->num_cus_, e->fast_);
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
    host_.reset(new HostPath(*this));
    return HashEngine::create(num_cus_, hash_);
}

const HostPlacement &Engine::placement() {
    if (!place_probed_) {
        place_ = HostPlacement::probe(device_);
        place_probed_ = true;
    }
    return place_;
}

Engine::~Engine() {
    if (device_ >= 0) (void)hipSetDevice(device_);
    if (in_flight()) (void)drain();
    walk_.reset();
    if (own_stream_) (void)hipStreamSynchronize(own_stream_);
    fast_.reset();
    hash_.reset();
    host_.reset();  // (its work ran on own_stream_, synchronised above and destroyed below)
    (void)hipFree(fixed_.d_block);
    (void)hipHostFree(fixed_.h_block);
    for (auto &ev : ev_)
        if (ev) (void)hipEventDestroy(ev);
    if (own_stream_) (void)hipStreamDestroy(own_stream_);
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
    if (host_->write_active()) {  // windows already chunked used the old table: a write never mixes two
        set_error("cdc_set_gear: a streaming write is in progress (cdc_write_finish it first)");
        return CDC_EINVAL;
    }
    HIP_TRY(hipSetDevice(device_));
    return fast_ ? fast_->set_gear(gear) : CDC_OK;  // (no other rule reads the table)
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
// handle completes the async batches first; FastEngine reports the ones its
// own calls had to make): its result -- the last batch's chunk count, or the
// error of a failed collection -- is what the next cdc_batch_sync returns.
void Engine::hold(int64_t result) {
    held_ = result;
    held_valid_ = true;
}

int64_t Engine::drain_implicit() {
    if (!in_flight()) return 0;
    hold(drain());
    return held_;
}

bool Engine::in_flight() const { return (fast_ && fast_->in_flight()) || (walk_ && walk_->in_flight()); }

int64_t Engine::drain() { return fast_ ? fast_->drain() : walk_ ? walk_->drain() : 0; }

int Engine::walk_params(uint64_t *v, size_t n) const { return walk_ ? walk_->debug_params(v, n) : -1; }

uint32_t Engine::record_cap() const { return fast_ ? fast_->record_cap() : 0; }

int64_t Engine::batch_device(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, cdc_chunk_t *d_out,
                             size_t out_cap, uint64_t *first, hipStream_t stream, bool async, bool skip_small) {
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
    // Multi-megabyte async batches go into the FastCDC pipeline or to the walk
    // contexts; everything else runs to completion here, after the batches in
    // flight.
    if (fast_) {
        int64_t drained = FastEngine::kNoDrain;
        const int64_t r = async && fast_->takes_async(n, bytes)
                              ? fast_->submit(n, d_streams, lens, d_out, out_cap, first, s, placement(), drained)
                              : fast_->chunk_batch(n, d_streams, lens, d_out, out_cap, first, s, placement(),
                                                   skip_small, drained);
        if (drained != FastEngine::kNoDrain) hold(drained);
        return r;
    }
    if (walk_ && async && walk_->takes_async(n, bytes))
        return walk_->submit(n, d_streams, lens, d_out, out_cap, first, s, placement());
    if (in_flight()) {
        const int64_t r = drain_implicit();
        if (r < 0) return r;
    }
    if (walk_) return walk_->chunk_batch(n, d_streams, lens, d_out, out_cap, first, s, placement());
    return run_fixed(n, d_streams, lens, bytes, d_out, first, s);
}

// ---- fixed-size path ------------------------------------------------------------

int Engine::ensure_fixed(size_t n) {
    Fixed &f = fixed_;
    if (f.streams >= n) return CDC_OK;
    (void)hipFree(f.d_block);
    (void)hipHostFree(f.h_block);
    f.d_block = f.h_block = nullptr;
    f.streams = 0;
    const size_t W = n + 64;  // per table: ptrs[W] lens[W] span_base[W+1] first[W+1]
    const size_t words = 4 * W + 2;
    HIP_TRY(placement().host_malloc(&f.h_block, words * sizeof(uint64_t), hipHostMallocCoherent));
    HIP_TRY(hipMalloc(&f.d_block, words * sizeof(uint64_t)));
    ++f.gen;
    uint64_t *h = static_cast<uint64_t *>(f.h_block), *d = static_cast<uint64_t *>(f.d_block);
    f.tab.h_ptrs = h;
    f.tab.h_lens = h + W;
    f.tab.h_sb = h + 2 * W;
    f.h_first = h + 3 * W + 1;
    f.tab.d_ptrs = reinterpret_cast<const uint8_t **>(d);
    f.tab.d_lens = d + W;
    f.tab.d_sb = d + 2 * W;
    f.d_first = d + 3 * W + 1;
    f.streams = W;
    return CDC_OK;
}

// One launch: the streams own no spans; ceil(len / chunk size) chunks each
// (fixed_size.rs:35-40), first[] computed here.
int64_t Engine::run_fixed(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, uint64_t bytes,
                          cdc_chunk_t *d_out, uint64_t *first, hipStream_t s) {
    cdc_timing_t empty{};
    empty.bytes = bytes;
    empty.path = CDC_PATH_EMPTY;
    report(empty);
    if (n == 0) {
        if (first) first[0] = 0;
        return 0;
    }
    Fixed &f = fixed_;
    int rc = ensure_fixed(n);
    if (rc) return rc;
    f.tab.fill(n, d_streams, lens, 0);
    StreamTable st;
    rc = f.tab.publish(n, bytes, 0, 0, f.gen, s, st);
    if (rc) return rc;
    uint64_t t = 0;
    for (size_t i = 0; i < n; ++i) {
        f.h_first[i] = t;
        t += (lens[i] + min_ - 1) / min_;
    }
    f.h_first[n] = t;
    HIP_TRY(hipEventRecord(ev_[0], s));
    HIP_TRY(hipMemcpyAsync(f.d_first, f.h_first, (n + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_fixed(st, min_, f.d_first, d_out, t, s));
    HIP_TRY(hipEventRecord(ev_[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(first, f.h_first, (n + 1) * 8);
    float t01 = 0;
    HIP_TRY(hipEventElapsedTime(&t01, ev_[0], ev_[1]));
    timing_.total_ms = t01;
    timing_.scan_ms = t01;
    timing_.path = CDC_PATH_FIXED;
    timing_.timed = 1;
    return (int64_t)first[n];
}

// ---- timing and debug entries ---------------------------------------------------

const cdc_timing_t &Engine::timing() {
    if (in_flight()) (void)drain_implicit();  // (a failure is held for the next cdc_batch_sync)
    if (fast_) report(fast_->timing());
    else if (walk_) report(walk_->timing());
    return timing_;
}

// A batch's timing as cdc_last_timing reports it: hash_ms stays the last
// hash call's (reported with the batch it hashed, until the next hash).
void Engine::report(const cdc_timing_t &batch) {
    const double hash_ms = timing_.hash_ms;
    timing_ = batch;
    timing_.hash_ms = hash_ms;
}

int Engine::timing_back(uint32_t back, cdc_timing_t &out) {
    if (in_flight()) (void)drain_implicit();
    if (!fast_) {
        set_error("cdc_debug_timing_back: no such FastCDC batch in the event ring");
        return CDC_EINVAL;
    }
    const int rc = fast_->timing_back(back, out);
    out.hash_ms = timing_.hash_ms;
    return rc;
}

int64_t Engine::debug_copy(int what, void *out, size_t max_bytes) {
    if (in_flight()) {
        const int64_t r = drain_implicit();
        if (r < 0) return r;
    }
    if (!fast_) {
        set_error("debug_copy: no FastCDC batch yet");
        return CDC_EINVAL;
    }
    HIP_TRY(hipSetDevice(device_));
    HIP_TRY(hipStreamSynchronize(own_stream_));
    return fast_->debug_copy(what, out, max_bytes);
}

// ---- the hashers, device utilities ----------------------------------------------------

int Engine::sha256_device(const uint8_t *d_data, const cdc_chunk_t *d_chunks, size_t n,
                          uint8_t *d_digests, hipStream_t s) {
    const uint64_t first[2] = {0, n};
    return hash_batch(CDC_HASH_SHA256, 1, &d_data, first, d_chunks, d_digests, s);
}

// One launch over every chunk of every stream (HashEngine::run).  `who` names
// the C entry point in the refusals.
int Engine::hash_batch(int hash, size_t n, const uint8_t *const *d_streams, const uint64_t *first,
                       const cdc_chunk_t *d_chunks, uint8_t *d_digests, hipStream_t s, const char *who) {
    if (n == 0) return CDC_OK;
    if (!d_streams || !first) {
        set_error(std::string(who) + ": NULL stream table");
        return CDC_EINVAL;
    }
    if (first[0] != 0) {
        set_error(std::string(who) + ": first[0] must be 0");
        return CDC_EINVAL;
    }
    for (size_t i = 0; i < n; ++i) {
        if (first[i + 1] < first[i]) {
            set_error(std::string(who) + ": first[] must be non-decreasing");
            return CDC_EINVAL;
        }
        if (first[i + 1] > first[i] && !d_streams[i]) {
            set_error(std::string(who) + ": NULL stream with chunks");
            return CDC_EINVAL;
        }
    }
    const uint64_t total = first[n];
    if (total >= (1ull << 32)) {
        set_error(std::string(who) + ": more than 2^32 - 1 chunks in one batch");
        return CDC_EINVAL;
    }
    if (total && (!d_chunks || !d_digests)) {
        set_error(std::string(hash == CDC_HASH_SHA256 ? "cdc_sha256_chunks_device" : who) + ": NULL argument");
        return CDC_EINVAL;
    }
    HIP_TRY(hipSetDevice(device_));
    if (in_flight()) {  // (the chunks it hashes are usually the last batch's)
        const int64_t r = drain_implicit();
        if (r < 0) return (int)r;
    }
    if (total == 0) {
        timing_.hash_ms = 0;
        return CDC_OK;
    }
    float ms = 0;
    const int rc = hash_->run(hash, n, d_streams, first, d_chunks, d_digests, total, s ? s : own_stream_, &ms);
    if (rc != CDC_OK) return rc;
    timing_.hash_ms = ms;
    return CDC_OK;
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
    if (e == hipSuccess) e = hipEventRecord(ev_[1], own_stream_);
    if (e == hipSuccess) e = hipEventSynchronize(ev_[1]);
    float t = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ev_[0], ev_[1]);
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
    if (host_->write_active()) {  // windows already chunked used the old polynomial: a write never mixes two
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
