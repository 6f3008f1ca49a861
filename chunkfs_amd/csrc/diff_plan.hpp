// diff_plan.hpp -- the index arithmetic of cdc_files_diff_device
// (include/chunkfs_amd.h, "Snapshots and diffs"), header-only and free of HIP so
// that a plain C++ program can run it under the host sanitizers
// (tools/diff_plan_check.cpp).  files.hip uses the same functions on the device.
//
// Three things live here: which span boundary of the two tables opens a piece
// and where that piece ranks (equal offsets -- length-0 spans, boundaries both
// tables have -- count once); the map between a bit of a tile's mask and a byte
// of the file; and the run starts and ends of one mask word with its carries.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CDC_DIFF_HD __host__ __device__ __forceinline__
#else
#define CDC_DIFF_HD inline
#endif

namespace cdc {

constexpr uint64_t kDiffTile = 4096;      // bytes (and mask bits) of one tile: the store's kStoreTile
constexpr uint32_t kDiffTileWords = 64;   // 64-bit mask words of one tile
constexpr uint64_t kDiffAlign = 16;       // tiles start at 16-byte multiples of the B side: the store's kStoreAlign

// First k in [0, entries) with off[k] >= x; `entries` when there is none.
CDC_DIFF_HD uint64_t diff_lower_bound(const uint64_t *off, uint64_t entries, uint64_t x) {
    uint64_t lo = 0, hi = entries;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The span that holds byte x < off[n]: the last k with off[k] <= x, which among
// equal offsets is the one span of them that has bytes.
CDC_DIFF_HD uint64_t diff_span_at(const uint64_t *off, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The two tables as one list of nA + nB + 2 candidates: candidate c <= nA is
// A's boundary off_a[c], candidate nA + 1 + j is B's boundary off_b[j].
CDC_DIFF_HD uint64_t diff_candidates(uint64_t na, uint64_t nb) { return na + nb + 2; }

// Does candidate c open a piece of [0, common)?  Every distinct boundary x <
// common has exactly one candidate that does: in a table, the last entry of
// that value (the span after it has bytes, x < common <= off[n]); between the
// tables, A's.  *x = the boundary.  common > 0, so both files have spans.
CDC_DIFF_HD bool diff_opens(const uint64_t *off_a, uint64_t na, const uint64_t *off_b, uint64_t nb, uint64_t common,
                            uint64_t c, uint64_t *x) {
    if (c <= na) {
        if (c == na || off_a[c] >= common || off_a[c + 1] == off_a[c]) return false;
        *x = off_a[c];
        return true;
    }
    const uint64_t j = c - na - 1;
    if (j >= nb || off_b[j] >= common || off_b[j + 1] == off_b[j]) return false;
    *x = off_b[j];
    const uint64_t k = diff_lower_bound(off_a, na + 1, *x);
    return !(k <= na && off_a[k] == *x);
}

// The rank of the piece candidate c opens, scan = the exclusive scan of
// diff_opens over the candidates: the openers before it in its own table plus
// those of the other table with a smaller boundary.  Also the piece's spans.
CDC_DIFF_HD uint64_t diff_rank(const uint64_t *off_a, uint64_t na, const uint64_t *off_b, uint64_t nb,
                               const uint64_t *scan, uint64_t c, uint64_t x, uint32_t *ia, uint32_t *ib) {
    const uint64_t b0 = na + 1;  // B's first candidate; scan[b0] = A's openers
    if (c <= na) {
        *ia = (uint32_t)c;
        *ib = (uint32_t)diff_span_at(off_b, nb, x);
        return scan[c] + (scan[b0 + diff_lower_bound(off_b, nb + 1, x)] - scan[b0]);
    }
    *ia = (uint32_t)diff_span_at(off_a, na, x);
    *ib = (uint32_t)(c - b0);
    return (scan[c] - scan[b0]) + scan[diff_lower_bound(off_a, na + 1, x)];
}

// The sharing rule: one slot at one file offset is one arena address.
CDC_DIFF_HD bool diff_shared(uint32_t slot_a, uint64_t start_a, uint32_t slot_b, uint64_t start_b) {
    return slot_a == slot_b && start_a == start_b;
}

// ---- tiles ------------------------------------------------------------------------
// A compared piece of len > 0 bytes whose B side lies at address dst is cut into
// tiles of kDiffTile bytes from dst & ~15 on: bit b of tile k stands for the
// address (dst & ~15) + k * kDiffTile + b.  m = dst & 15.
CDC_DIFF_HD uint64_t diff_tiles(uint64_t dst, uint64_t len) {
    return len ? ((dst & (kDiffAlign - 1)) + len + (kDiffTile - 1)) / kDiffTile : 0;
}
// The file offset of bit b of tile k of a piece that starts at file offset x.
CDC_DIFF_HD uint64_t diff_file_offset(uint64_t x, uint32_t m, uint64_t k, uint32_t b) {
    return x + k * kDiffTile + b - m;
}
// Where the piece's last byte lies: tile *k, bit *b.
CDC_DIFF_HD void diff_last_bit(uint32_t m, uint64_t len, uint64_t *k, uint32_t *b) {
    const uint64_t pos = m + len - 1;
    *k = pos / kDiffTile;
    *b = (uint32_t)(pos % kDiffTile);
}

// ---- runs ------------------------------------------------------------------------
// Bits of w that begin a run: set, with the bit before clear.  prev = the bit
// before bit 0.  Likewise the bits that end one; next = the bit after bit 63.
CDC_DIFF_HD uint64_t diff_word_starts(uint64_t w, uint64_t prev) { return w & ~((w << 1) | (prev & 1)); }
CDC_DIFF_HD uint64_t diff_word_ends(uint64_t w, uint64_t next) { return w & ~((w >> 1) | ((next & 1) << 63)); }

// One tile of a compared piece, as the run passes see it.  Bits outside the
// piece are clear, so a piece's first and last byte begin and end a run by the
// word rule alone; the two flags take that back where the run goes on in the
// neighbouring piece (adjacent in the file and compared, its border byte
// differing) or in the tail past `common`.
struct DiffTile {
    uint32_t m;        // dst & 15 of the piece
    uint64_t len;      // of the piece
    uint64_t k;        // this tile of the piece
    bool head_joined;  // the piece's first byte continues a run
    bool tail_joined;  // a run through the piece's last byte goes on
};

// Run starts of word l (0..63) of the tile.  prev = bit 63 of the word before
// it in the piece's mask (0 for the piece's first word).
CDC_DIFF_HD uint64_t diff_tile_starts(const DiffTile &t, uint32_t l, uint64_t w, uint64_t prev) {
    uint64_t s = diff_word_starts(w, prev);
    if (t.k == 0 && l == 0 && t.head_joined) s &= ~(1ull << t.m);
    return s;
}
// Run ends of word l.  next = bit 0 of the word after it in the piece's mask (0
// for the piece's last word).
CDC_DIFF_HD uint64_t diff_tile_ends(const DiffTile &t, uint32_t l, uint64_t w, uint64_t next) {
    uint64_t e = diff_word_ends(w, next);
    uint64_t k;
    uint32_t b;
    diff_last_bit(t.m, t.len, &k, &b);
    if (t.tail_joined && t.k == k && l == b / 64) e &= ~(1ull << (b % 64));
    return e;
}
// 1 when a run that began before the tile goes on into it: the tile's first
// byte differs and begins no run.  The ends before a tile are the starts
// before it less this.
CDC_DIFF_HD uint64_t diff_tile_open(const DiffTile &t, uint64_t w0, uint64_t starts0) {
    const uint32_t fb = t.k == 0 ? t.m : 0;
    return ((w0 >> fb) & 1) & ~((starts0 >> fb) & 1);
}

}  // namespace cdc
