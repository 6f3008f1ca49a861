// splice_plan.hpp -- the index arithmetic of cdc_file_splice_device
// (include/chunkfs_amd.h, "Editing a file in place"), header-only and free of
// HIP so that a plain C++ program can run it under the host sanitizers
// (tools/splice_plan_check.cpp).  files.hip uses the same functions on the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CDC_SPLICE_HD __host__ __device__ __forceinline__
#else
#define CDC_SPLICE_HD inline
#endif

namespace cdc {

// Bytes a chunker may read at or past a cut: AE's cut after byte i reads the
// bytes i .. i+3; 8 leaves room and keeps the start span's rule one number.
constexpr uint64_t kSpliceBack = 8;

CDC_SPLICE_HD uint64_t splice_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
CDC_SPLICE_HD uint64_t splice_sat_mul(uint64_t a, uint64_t b) { return b && a > ~0ull / b ? ~0ull : a * b; }

// The argument check: the range [offset, offset + remove_len) lies inside the file.
CDC_SPLICE_HD bool splice_range_ok(uint64_t size, uint64_t offset, uint64_t remove_len) {
    return offset <= size && remove_len <= size - offset;
}

// size + insert_len - remove_len; false when it does not fit 64 bits.
CDC_SPLICE_HD bool splice_size_after(uint64_t size, uint64_t remove_len, uint64_t insert_len, uint64_t *out) {
    const uint64_t kept = size - remove_len;
    if (kept + insert_len < kept) return false;
    *out = kept + insert_len;
    return true;
}

// Step 1: the last span i in [0, n) with off[i] + 8 <= offset, among equal
// offsets the last; 0 if there is none (or no span).  off: n + 1 entries.
CDC_SPLICE_HD uint64_t splice_start_span(const uint64_t *off, uint64_t n, uint64_t offset) {
    if (n == 0 || offset < kSpliceBack) return 0;
    const uint64_t x = offset - kSpliceBack;  // off[0] = 0 <= x
    uint64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Where round `round` (1, 2, ...) stops chunking: the look-ahead beyond the
// inserted bytes is 4^round * max + 8, clipped to the new file.
CDC_SPLICE_HD uint64_t splice_window_end(uint64_t size_after, uint64_t offset, uint64_t insert_len, uint64_t max_chunk,
                                         uint32_t round) {
    uint64_t look = max_chunk;
    for (uint32_t r = 0; r < round && look != ~0ull; ++r) look = splice_sat_mul(look, 4);
    const uint64_t end = splice_sat_add(splice_sat_add(offset, insert_len), splice_sat_add(look, kSpliceBack));
    return end < size_after ? end : size_after;
}

// A chunk of a window that starts at `start` (file coordinates) equals the chunk
// the whole tail would give: everything it can depend on lies inside the window,
// or the window ends where the file does.
CDC_SPLICE_HD bool splice_trusted(uint64_t start, uint64_t max_chunk, uint64_t end_w, uint64_t size_after) {
    if (end_w == size_after) return true;
    const uint64_t need = splice_sat_add(splice_sat_add(start, max_chunk), kSpliceBack);
    return need <= end_w;
}

// Step 3 for one cut e >= offset + insert_len: the smallest j in [0, n] with
// off[j] == e - delta; false if that is no old boundary.  A file without spans
// has the one boundary 0.
CDC_SPLICE_HD bool splice_old_boundary(const uint64_t *off, uint64_t n, uint64_t e, uint64_t remove_len,
                                       uint64_t insert_len, uint64_t *j) {
    const uint64_t x = e - insert_len + remove_len;
    if (n == 0) {
        *j = 0;
        return x == 0;
    }
    uint64_t lo = 0, hi = n + 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    *j = lo;
    return lo <= n && off[lo] == x;
}

}  // namespace cdc
