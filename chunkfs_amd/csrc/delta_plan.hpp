// delta_plan.hpp -- the index arithmetic of cdc_files_delta_device
// (include/chunkfs_amd.h, "Content-aligned delta"), header-only and free of HIP
// so that a plain C++ program can run it under the host sanitizers
// (tools/delta_plan_check.cpp).  delta.hip uses the same functions on the device.
//
// Five things live here: the nearest-offset search inside one slot's group of
// the sorted (slot, span) pairs, with its tie rule; where byte x of a region
// lies in the other file (the region's shift, then the span that holds it); the
// map from a tile of the edge pass to a byte range of its region; the clip of
// the backward match; and which ops of a run open an op of the canonical script.
#pragma once
#include <stdint.h>

#include "diff_plan.hpp"

namespace cdc {

constexpr uint64_t kDeltaTile = 4096;  // bytes of B one block of the edge pass compares, per direction
constexpr uint32_t kDeltaSeg = 16;     // bytes of a tile one thread compares
constexpr int64_t kDeltaNone = INT64_MIN;      // a span of B that no span of A matches; a LITERAL run
constexpr int64_t kDeltaSkip = INT64_MIN + 1;  // a span of length 0: it holds no byte and takes no part

// ---- anchors ----------------------------------------------------------------------
// key[0, n) ascending: the slots of A's spans after the stable sort.  [*g0, *g1)
// = the entries equal to slot.
CDC_DIFF_HD void delta_group(const uint64_t *key, uint64_t n, uint64_t slot, uint64_t *g0, uint64_t *g1) {
    *g0 = diff_lower_bound(key, n, slot);
    *g1 = diff_lower_bound(key, n, slot + 1);
}

// idx[g0, g1), g0 < g1: span indices of A in ascending order, all of one slot
// and of one length > 0, so off_a[idx[.]] strictly ascends.  The span that
// minimises |off_a[i] - x|; on a tie the smaller off_a[i].
CDC_DIFF_HD uint32_t delta_nearest(const uint64_t *off_a, const uint32_t *idx, uint64_t g0, uint64_t g1, uint64_t x) {
    uint64_t lo = g0, hi = g1;  // first p with off_a[idx[p]] >= x
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off_a[idx[mid]] < x) lo = mid + 1;
        else hi = mid;
    }
    if (lo == g1) return idx[g1 - 1];
    if (lo == g0) return idx[g0];
    const uint64_t above = off_a[idx[lo]] - x, below = x - off_a[idx[lo - 1]];
    return above < below ? idx[lo] : idx[lo - 1];
}

// The diagonal of a match: A's offset less B's, as a two's complement difference.
CDC_DIFF_HD int64_t delta_diagonal(uint64_t off_a, uint64_t off_b) { return (int64_t)(off_a - off_b); }

// ---- regions ------------------------------------------------------------------------
// One LITERAL run of B after step 2, set against its neighbours' diagonals.
struct DeltaRegion {
    uint64_t l, r;   // B's bytes [l, r), l < r
    int64_t dl, dr;  // the left COPY's diagonal (0 at the file's start), the right one's (size_a - size_b at its end)
};

// How far the forward match may run: r - l, cut where l + dl + k leaves [0, size_a).
CDC_DIFF_HD uint64_t delta_fwd_cap(const DeltaRegion &g, uint64_t size_a) {
    const int64_t a0 = (int64_t)g.l + g.dl;
    if (a0 < 0 || (uint64_t)a0 >= size_a) return 0;
    const uint64_t room = size_a - (uint64_t)a0, len = g.r - g.l;
    return room < len ? room : len;
}
// The lowest x of [l, r] from which the backward match may hold down to: x + dr
// stays inside [0, size_a) for every x in [floor, r).  r when no byte qualifies.
CDC_DIFF_HD uint64_t delta_bwd_floor(const DeltaRegion &g, uint64_t size_a) {
    const int64_t top = (int64_t)g.r + g.dr;  // A's index one past the last byte
    if (top <= 0 || (uint64_t)top > size_a) return g.r;
    uint64_t lo = g.l;
    if (g.dr < 0 && (uint64_t)(-g.dr) > lo) lo = (uint64_t)(-g.dr);
    return lo < g.r ? lo : g.r;
}

// Tiles of a region: the same count serves both directions.
CDC_DIFF_HD uint64_t delta_tiles(uint64_t len) { return (len + kDeltaTile - 1) / kDeltaTile; }
// Forward tile t counts from l, backward tile t from r: block t of a region
// takes both, so the first blocks hold the bytes either search meets first.
CDC_DIFF_HD void delta_fwd_tile(const DeltaRegion &g, uint64_t t, uint64_t *x0, uint64_t *x1) {
    *x0 = g.l + t * kDeltaTile;
    *x1 = g.r - *x0 < kDeltaTile ? g.r : *x0 + kDeltaTile;
}
CDC_DIFF_HD void delta_bwd_tile(const DeltaRegion &g, uint64_t t, uint64_t *x0, uint64_t *x1) {
    *x1 = g.r - t * kDeltaTile;
    *x0 = *x1 - g.l < kDeltaTile ? g.l : *x1 - kDeltaTile;
}
// The bytes of [x0, x1) thread `lane` compares, clipped to [lo, hi).  Forward
// segments count from x0, backward ones from x1.
CDC_DIFF_HD bool delta_segment(uint64_t x0, uint64_t x1, uint32_t lane, bool backward, uint64_t lo, uint64_t hi,
                               uint64_t *s0, uint64_t *s1) {
    const uint64_t skip = (uint64_t)lane * kDeltaSeg;
    if (skip >= x1 - x0) return false;
    if (!backward) {
        *s0 = x0 + skip;
        *s1 = x1 - *s0 < kDeltaSeg ? x1 : *s0 + kDeltaSeg;
    } else {
        *s1 = x1 - skip;
        *s0 = *s1 - x0 < kDeltaSeg ? x0 : *s1 - kDeltaSeg;
    }
    if (*s0 < lo) *s0 = lo;
    if (*s1 > hi) *s1 = hi;
    return *s0 < *s1;
}

// Byte x of B under the diagonal d is A's byte x + d.
CDC_DIFF_HD uint64_t delta_a_index(uint64_t x, int64_t d) { return x + (uint64_t)d; }

// ---- clip ---------------------------------------------------------------------------
// e = the forward match, back = the full backward match: forward takes
// precedence, and a suffix match is monotone, so f = min(back, len - e).
CDC_DIFF_HD uint64_t delta_clip(uint64_t len, uint64_t e, uint64_t back) { return back < len - e ? back : len - e; }

// ---- canonical form -------------------------------------------------------------------
// Two neighbouring ops are one when both are COPYs on one diagonal.
CDC_DIFF_HD bool delta_merges(bool prev_copy, int64_t prev_d, bool copy, int64_t d) {
    return prev_copy && copy && prev_d == d;
}

// A region gives COPY e (diagonal dl), LITERAL len - e - f, COPY f (diagonal
// dr).  Which of the three open an op of the script: bit 0, 1, 2.  The op
// before the region is the left COPY run, on dl, when has_left.
CDC_DIFF_HD uint32_t delta_region_heads(uint64_t len, uint64_t e, uint64_t f, int64_t dl, int64_t dr, bool has_left) {
    const uint64_t lit = len - e - f;
    uint32_t heads = 0;
    if (e && !has_left) heads |= 1u;  // after a COPY run the prefix continues it
    if (lit) heads |= 2u;
    if (f && !(lit == 0 && delta_merges(e || has_left, dl, true, dr))) heads |= 4u;
    return heads;
}
// Does the COPY run on diagonal d open an op, after a region {len, e, f, dl}?
// Its suffix is on d already; past a vanished literal the op before is on dl.
CDC_DIFF_HD bool delta_copy_head_after_region(uint64_t len, uint64_t e, uint64_t f, int64_t dl, int64_t d) {
    if (f) return false;
    if (len - e) return true;
    return !delta_merges(true, dl, true, d);
}

}  // namespace cdc
