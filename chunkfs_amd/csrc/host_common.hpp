// host_common.hpp -- what the host classes behind the C ABI share (Engine,
// FastEngine, WalkEngine, HostPath, the store and the file layer): the error
// text, HIP_TRY, the owned grow-only buffers, the pinned-memory placement, the
// copy pool and the per-call stream tables.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/chunkfs_amd.h"
#include "cdc_kernels.hpp"

namespace cdc {

void set_error(const std::string &msg);
const char *last_error();

#define HIP_TRY(expr)                                                          \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) {                                                \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));      \
            return CDC_EDEVICE;                                                \
        }                                                                      \
    } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline uint32_t ceil_log2(uint64_t x) {
    uint32_t r = 0;
    while ((1ull << r) < x) ++r;
    return r;
}

// Memory an object keeps between calls: `cap` elements of T on the device, or
// pinned on the host, freed with its owner (with the owner's device current).
// room() leaves a buffer that is large enough alone; otherwise it frees it and
// allocates exactly `count` elements, the contents are not kept.  How much to
// ask for is the caller's rule.  After a failure the buffer is empty.
template <typename T, bool kPinned>
struct Owned {
    T *p = nullptr;
    uint64_t cap = 0;
    Owned() = default;
    Owned(Owned &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }  // move-only: no copies
    ~Owned() { drop(); }
    void drop() {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr, cap = 0;
    }
    hipError_t room(uint64_t count) {
        if (cap >= count) return hipSuccess;
        drop();
        void *q = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&q, count * sizeof(T)) : hipMalloc(&q, count * sizeof(T));
        if (e == hipSuccess) p = static_cast<T *>(q), cap = count;
        return e;
    }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};
template <typename T>
using DeviceBuf = Owned<T, false>;
template <typename T>
using PinnedBuf = Owned<T, true>;

// Buffers that grow together, `cap` what the group holds: nothing to do while
// cap >= n; else room(count) for each {buffer, count} pair up to the first
// failure, and cap = to -- or 0 after a failure: the next call allocates again.
inline hipError_t room_all() { return hipSuccess; }
template <typename B, typename... R>
hipError_t room_all(B &buf, uint64_t count, R &&...rest) {
    const hipError_t e = buf.room(count);
    return e == hipSuccess ? room_all(rest...) : e;
}
template <typename... A>
hipError_t grow_group(uint64_t &cap, uint64_t n, uint64_t to, A &&...pairs) {
    if (cap >= n) return hipSuccess;
    cap = 0;
    const hipError_t e = room_all(pairs...);
    if (e == hipSuccess) cap = to;
    return e;
}

// Where the host side of the boundary runs (hostpath.cpp): the device's PCIe
// address, NUMA node and link; the node's CPUs this process may use.
struct HostPlacement {
    std::string pci, link, link_max;
    int node = -1;
    int allowed = 0;          // CPUs in this process's affinity mask
    std::vector<int> cpus;    // of them, those on `node`
    bool enabled = false;     // pinned memory and copy helpers placed on `node`
    static HostPlacement probe(int device);
    hipError_t host_malloc(void **ptr, size_t bytes, unsigned flags) const;
    static int node_of(const void *addr);  // NUMA node of the page at addr (-1: unknown)
};

// Pageable -> pinned copies of the host path split over a few threads (one
// core copies ~20 GB/s, below what the H2D DMA takes).  One pool per process
// (CopyPool::shared), helpers spin briefly after a job (the next 1 MiB segment
// usually follows within microseconds), then sleep.  copy() returns when
// every part is done (hostpath.cpp).
class CopyPool {
  public:
    CopyPool(unsigned threads, unsigned spin_us, const std::vector<int> &cpus);
    ~CopyPool();
    static CopyPool &for_node(int node, const std::vector<int> &cpus);
    void copy(void *dst, const void *src, size_t n);
    // Streamed copy for the small kernel's feed: pieces of `piece` bytes,
    // claimed by the caller and the awake helpers, each announced by
    // ready[piece index] = seq once copied (the device reads it over PCIe
    // while later pieces are still being copied).  Returns once every piece
    // is announced.
    void copy_feed(void *dst, const void *src, size_t n, size_t piece, volatile uint64_t *ready, uint64_t seq);
    unsigned threads() const { return (unsigned)th_.size() + 1; }
    unsigned pinned() const { return pinned_; }

  private:
    void run(unsigned id);
    void work();  // claim and copy pieces until none is left
    void job(void *dst, const void *src, size_t n, size_t piece, volatile uint64_t *ready, uint64_t seq);
    std::vector<std::thread> th_;
    std::mutex m_, job_m_;
    std::condition_variable cv_;
    unsigned spin_us_ = 200;
    unsigned pinned_ = 0;  // helpers bound to the node's CPUs
    std::atomic<uint64_t> gen_{0};
    std::atomic<bool> stop_{false}, open_{false};
    std::atomic<unsigned> active_{0};  // helpers inside the current job
    std::atomic<size_t> next_{0}, done_{0};  // next piece to claim, pieces copied
    uint8_t *dst_ = nullptr;
    const uint8_t *src_ = nullptr;
    size_t n_ = 0, piece_ = 0, np_ = 0;
    volatile uint64_t *ready_ = nullptr;  // feed words (nullptr: a plain copy)
    uint64_t seq_ = 0;
};

// Batches of more than kSmallBatch bytes are the ones the async entry
// pipelines (FastCDC) or hands to a context (segment walk).
constexpr uint64_t kSmallBatch = uint64_t(8) << 20;
// Batches this small with few streams read their stream tables straight
// from the pinned staging block (no H2D copies: each small copy costs a
// ~10 us DMA on the call's critical path).
constexpr size_t kZeroCopyStreams = 64;

// One call's stream tables (walk and fixed-size paths): staged in pinned,
// coherent host memory (h_*), with device copies (d_*) for the batches that
// do not read the host block itself.  `last` / `last_gen` remember what was
// uploaded into which workspace generation, to skip unchanged H2D copies.
struct CallTables {
    uint64_t *h_ptrs = nullptr, *h_lens = nullptr, *h_sb = nullptr;  // [n] [n] [n+1]
    const uint8_t **d_ptrs = nullptr;
    uint64_t *d_lens = nullptr, *d_sb = nullptr;
    std::vector<uint64_t> last;  // ptrs ++ lens as last uploaded
    uint64_t last_gen = ~0ull;

    // Fills the host tables; span_log2 0: the streams own no spans.  Returns
    // the batch's spans.
    uint64_t fill(size_t n, const uint8_t *const *d_streams, const uint64_t *lens, uint32_t span_log2) {
        uint64_t spans = 0;
        for (size_t i = 0; i < n; ++i) {
            h_ptrs[i] = reinterpret_cast<uint64_t>(d_streams[i]);
            h_lens[i] = lens[i];
            h_sb[i] = spans;
            if (span_log2) spans += (lens[i] + (1ull << span_log2) - 1) >> span_log2;
        }
        h_sb[n] = spans;
        return spans;
    }
    // The table the kernels read.  Small batches (the host path's per-segment
    // calls) read the pinned block itself: the kernels' few table loads cross
    // PCIe, but no copy sits on the call's critical path.  Larger batches
    // re-upload the three per-stream tables only when they changed or the
    // workspace (generation `gen`) moved: repeated batches over the same
    // device buffers skip the H2D copies.
    int publish(size_t n, uint64_t bytes, uint32_t span_log2, uint64_t spans, uint64_t gen, hipStream_t s,
                StreamTable &st) {
        const bool zero_copy = bytes <= kSmallBatch && n <= kZeroCopyStreams;
        const bool same = zero_copy || (gen == last_gen && last.size() == 2 * n &&
                                        std::memcmp(last.data(), h_ptrs, n * 8) == 0 &&
                                        std::memcmp(last.data() + n, h_lens, n * 8) == 0);
        if (!same) {
            HIP_TRY(hipMemcpyAsync(d_ptrs, h_ptrs, n * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_lens, h_lens, n * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_sb, h_sb, (n + 1) * 8, hipMemcpyHostToDevice, s));
            last.assign(h_ptrs, h_ptrs + n);
            last.insert(last.end(), h_lens, h_lens + n);
            last_gen = gen;
        }
        st = StreamTable{};
        st.ptrs = zero_copy ? reinterpret_cast<const uint8_t *const *>(h_ptrs) : d_ptrs;
        st.lens = zero_copy ? h_lens : d_lens;
        st.span_base = zero_copy ? h_sb : d_sb;
        st.n = (uint32_t)n;
        st.span_log2 = span_log2;
        st.total_spans = spans;
        return CDC_OK;
    }
};

}  // namespace cdc
