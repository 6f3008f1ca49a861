// read_plan.hpp -- the arithmetic of the file layer's range planner
// (include/chunkfs_amd.h, "File layer"), header-only and free of HIP so that a
// plain C++ program can run it under the host sanitizers
// (tools/read_plan_check.cpp).  files.hip resolves every request with it;
// files_host.cpp sizes grids and scratch from its bounds before the first
// launch, where a bound below the true count would drop pieces.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CDC_READ_HD __host__ __device__ __forceinline__
#else
#define CDC_READ_HD inline
#endif

namespace cdc {

constexpr uint64_t kReadTile = 4096;  // destination bytes of one copy tile: the store's kStoreTile
constexpr uint64_t kReadAlign = 16;   // tiles start at 16-byte multiples of the destination: the store's kStoreAlign

enum ReadKind : uint32_t {
    kReadComplete = 0,  // every span: read_file_complete
    kReadSegment = 1,   // whole spans from the cursor while their total stays <= seg: read_from_file
    kReadRange = 2,     // the bytes [a, a + b) clipped to the file: pread
};

// First i in [0, n) with off[i] >= x (n when there is none): the reference's
// skip_while(span.offset < handle.offset).
CDC_READ_HD uint64_t first_at_or_after(const uint64_t *__restrict__ off, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Largest k in [lo, hi] with off[k] <= x; off[lo] <= x must hold.  Equal
// offsets (length-0 spans) resolve to the last of them.
CDC_READ_HD uint64_t last_at_or_before(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// What a request resolves to: the bytes [lo, hi) of the file and the `count`
// spans from `first` on that hold them.
struct ReadSpans {
    uint64_t lo, hi, first, count;
};
// One request of `kind` over a table of n spans (off: n + 1 entries).  a, b: the
// segment read's cursor and segment size, the range read's offset and length.
// A destination of cap < hi - lo bytes copies nothing: count = 0.
CDC_READ_HD ReadSpans read_resolve(const uint64_t *__restrict__ off, uint64_t n, uint32_t kind, uint64_t a, uint64_t b,
                                   uint64_t cap) {
    uint64_t lo = 0, hi = 0, first = 0, count = 0;
    if (n) {
        const uint64_t size = off[n];
        if (kind == kReadComplete) {
            hi = size;
            count = n;
        } else if (kind == kReadSegment) {
            const uint64_t i0 = first_at_or_after(off, n, a);
            if (i0 < n) {
                lo = off[i0];
                const uint64_t limit = lo + b < lo ? ~0ull : lo + b;
                // take_while(running total <= segment): the largest k with off[k] - off[i0] <= seg.
                const uint64_t k = last_at_or_before(off, i0, n, limit);
                hi = off[k];
                first = i0;
                count = k - i0;
            }
        } else {
            lo = a < size ? a : size;
            hi = b > size - lo ? size : lo + b;
            if (hi > lo) {
                // lo < size = off[n]: the span that holds byte lo is the last one starting at or before it.
                first = last_at_or_before(off, 0, n, lo);
                count = last_at_or_before(off, first, n, hi - 1) - first + 1;
            }
        }
    }
    if (hi - lo > cap) count = 0;
    return ReadSpans{lo, hi, first, count};
}

// Spans a range of at most `bytes` bytes can touch, whole spans but for its two
// ends, in a file of n spans of which `zeros` have length 0 and the shortest
// other one min_len bytes (~0: there is none): the spans of length 0, the longer
// ones that fit, and the two ends.
CDC_READ_HD uint64_t spans_bound(uint64_t n, uint64_t min_len, uint64_t zeros, uint64_t bytes) {
    const uint64_t fit = min_len == ~0ull ? 0 : bytes / min_len;
    const uint64_t bound = zeros + fit + 2;
    return bound < n ? bound : n;
}

// The host's bound on one request before it is resolved: at most `bytes` bytes
// copied and `spans` spans touched (also without bytes: length-0 spans are
// pieces).  b as in read_resolve, size = off[n].
struct ReadBound {
    uint64_t bytes, spans;
};
CDC_READ_HD ReadBound read_bound(uint32_t kind, uint64_t b, uint64_t cap, uint64_t n, uint64_t size, uint64_t min_len,
                                 uint64_t zeros) {
    uint64_t bytes = size < cap ? size : cap;
    if (kind != kReadComplete && b < bytes) bytes = b;
    return ReadBound{bytes, kind == kReadComplete ? n : spans_bound(n, min_len, zeros, bytes)};
}

// Tiles of `pieces` pieces holding `bytes` bytes in all: a piece adds at most
// two ragged tiles to its whole ones.
CDC_READ_HD uint64_t read_tiles_bound(uint64_t bytes, uint64_t pieces) { return bytes / kReadTile + 2 * pieces; }

}  // namespace cdc
