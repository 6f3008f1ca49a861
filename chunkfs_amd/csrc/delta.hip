// delta.hip -- cdc_files_delta_device on the device (not in the reference;
// DESIGN.md "Content-aligned delta"): an edit script that builds file B out of
// file A, aligned by content.
//
// The store is content-defined, so the tables give the alignment: A's (slot,
// span) pairs are sorted; one thread per span of B finds its slot's group and in
// it the span of A nearest in offset, which gives the span's diagonal; spans of
// one diagonal in a row are a COPY run, unmatched ones a LITERAL region.  Exact
// mode then sets every region against its neighbours' diagonals: one block per
// 4 KiB of a region compares those bytes of B with A under the left diagonal
// (first mismatch, counted from the region's start) and the bytes the same
// distance from the region's end under the right one (last mismatch).  A block
// whose bytes lie past what is already known returns without reading, and only
// a block that improves a region's word issues an atomic.  The ops are flagged
// per run, scanned and emitted in canonical form.  The arithmetic is
// delta_plan.hpp's.
#include "delta.hpp"

#include "delta_plan.hpp"

namespace cdc {
namespace {

constexpr int kDlThreads = 256;
constexpr unsigned kDlMaxBlocks = 1u << 18;  // blocks of the edge pass past this stride
static_assert(kDlThreads * kDeltaSeg == kDeltaTile, "one thread per segment of a tile");

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kDlThreads - 1) / kDlThreads); }

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) v += __shfl_xor(v, k);
    return v;
}
// acc += the wave's sum; every lane of the wave calls it.
__device__ __forceinline__ void wave_add(unsigned long long *acc, uint64_t v) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(acc, (unsigned long long)v);
}
__device__ __forceinline__ unsigned long long peek(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Stage 1: the pairs the sort takes.
__global__ __launch_bounds__(kDlThreads) void delta_key_kernel(const uint32_t *__restrict__ slot, uint64_t na,
                                                               uint64_t *key, uint32_t *idx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= na) return;
    key[i] = slot[i];
    idx[i] = (uint32_t)i;
}

// Stage 2: one thread per span of B.
__global__ __launch_bounds__(kDlThreads) void delta_match_kernel(DiffSide a, DiffSide b,
                                                                 const uint64_t *__restrict__ key,
                                                                 const uint32_t *__restrict__ idx, int64_t *diag,
                                                                 unsigned long long *acc) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t matched = 0;
    if (j < b.n) {
        int64_t d = kDeltaSkip;
        if (b.off[j + 1] != b.off[j]) {
            uint64_t g0, g1;
            delta_group(key, a.n, b.slot[j], &g0, &g1);
            d = kDeltaNone;
            if (g0 < g1) {
                d = delta_diagonal(a.off[delta_nearest(a.off, idx, g0, g1, b.off[j])], b.off[j]);
                matched = 1;
            }
        }
        diag[j] = d;
    }
    wave_add(acc + 2, matched);
}

// Stage 3a: span j begins a run when it holds bytes and the span with bytes
// before it has another diagonal (two unmatched spans have the same: none).
__global__ __launch_bounds__(kDlThreads) void delta_flag_kernel(DiffSide b, const int64_t *__restrict__ diag,
                                                                uint64_t *rflag) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b.n) return;
    uint64_t f = 0;
    if (diag[j] != kDeltaSkip) f = b.off[j] == 0 || diag[diff_span_at(b.off, b.n, b.off[j] - 1)] != diag[j];
    rflag[j] = f;
}

// Stage 3b, after the scan: the run heads, closed by size_b.
__global__ __launch_bounds__(kDlThreads) void delta_run_kernel(DiffSide b, const int64_t *__restrict__ diag,
                                                               DeltaScratch w) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) {
        w.rb[*w.n_runs] = b.size;
        w.rd[*w.n_runs] = kDeltaSkip;
    }
    if (j >= b.n) return;
    const uint64_t next = j + 1 < b.n ? w.rflag[j + 1] : *w.n_runs;
    if (next == w.rflag[j]) return;  // the exclusive scan steps where a run begins
    w.rb[w.rflag[j]] = b.off[j];
    w.rd[w.rflag[j]] = diag[j];
}

__device__ __forceinline__ DeltaRegion region_of(const DeltaScratch &w, uint64_t k, uint64_t n_runs, uint64_t size_a,
                                                 uint64_t size_b) {
    DeltaRegion g;
    g.l = w.rb[k];
    g.r = w.rb[k + 1];
    g.dl = k ? w.rd[k - 1] : 0;
    g.dr = k + 1 < n_runs ? w.rd[k + 1] : (int64_t)(size_a - size_b);
    return g;
}

// Stage 3c: per run its tiles and, for a region, the two words the edge pass
// improves.  Tables only: no tile, and the words say that nothing matched.
__global__ __launch_bounds__(kDlThreads) void delta_region_kernel(uint64_t size_a, uint64_t size_b, uint64_t nb,
                                                                  bool tables_only, DeltaScratch w) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_runs = *w.n_runs;
    uint64_t bytes = 0, regions = 0;
    if (k < nb) {
        uint64_t tiles = 0;
        if (k < n_runs && w.rd[k] == kDeltaNone) {
            const DeltaRegion g = region_of(w, k, n_runs, size_a, size_b);
            bytes = g.r - g.l;
            regions = 1;
            if (tables_only) {
                w.fwd[k] = 0;
                w.bwd[k] = g.r;
            } else {
                w.fwd[k] = delta_fwd_cap(g, size_a);
                w.bwd[k] = delta_bwd_floor(g, size_a);
                tiles = delta_tiles(bytes);
            }
        }
        w.tstart[k] = tiles;
    }
    wave_add(w.acc + 1, bytes);
    wave_add(w.acc + 3, regions);
}

// ---- the edge pass ---------------------------------------------------------------------
// B's bytes [s0, s1), at most kDeltaSeg of them, against A's under diagonal d;
// every byte of either side lies inside its file.  *first / *last = the lowest
// and highest x that differ, ~0 when none does.  Both sides are sequences of
// spans at unrelated arena addresses: a segment inside one span of either side
// is two 16-byte loads of exactly its bytes, any other goes byte by byte, so no
// load touches a byte outside the spans' own.
__device__ __forceinline__ void seg_compare(const DiffSide &a, const DiffSide &b, const uint8_t *__restrict__ arena,
                                            uint64_t s0, uint64_t s1, int64_t d, uint64_t *first, uint64_t *last) {
    *first = *last = ~0ull;
    const uint64_t y0 = delta_a_index(s0, d);
    uint64_t jb = diff_span_at(b.off, b.n, s0), ia = diff_span_at(a.off, a.n, y0);
    uint64_t eb = b.off[jb + 1], ea = a.off[ia + 1];
    const uint8_t *pb = arena + b.loc[jb] + (s0 - b.off[jb]);
    const uint8_t *pa = arena + a.loc[ia] + (y0 - a.off[ia]);
    if (s1 - s0 == kDeltaSeg && s1 <= eb && y0 + kDeltaSeg <= ea) {
        uint64_t vb[2], va[2];
        __builtin_memcpy(vb, pb, 16);
        __builtin_memcpy(va, pa, 16);
        const uint64_t lo = vb[0] ^ va[0], hi = vb[1] ^ va[1];
        if (lo | hi) {
            *first = s0 + (lo ? (uint64_t)__builtin_ctzll(lo) / 8 : 8 + (uint64_t)__builtin_ctzll(hi) / 8);
            *last = s0 + (hi ? 15 - (uint64_t)__builtin_clzll(hi) / 8 : 7 - (uint64_t)__builtin_clzll(lo) / 8);
        }
        return;
    }
    for (uint64_t x = s0; x < s1; ++x, ++pb, ++pa) {
        if (x == eb) {  // the next span with bytes: x < size_b, so there is one
            do ++jb;
            while (b.off[jb + 1] == x);
            eb = b.off[jb + 1];
            pb = arena + b.loc[jb];
        }
        if (delta_a_index(x, d) == ea) {
            do ++ia;
            while (a.off[ia + 1] == ea);
            ea = a.off[ia + 1];
            pa = arena + a.loc[ia];
        }
        if (*pb != *pa) {
            if (*first == ~0ull) *first = x;
            *last = x;
        }
    }
}

// One block per tile of the tile scan: forward tile t of its region and
// backward tile t, 16 bytes per thread either way.
__global__ __launch_bounds__(kDlThreads) void delta_edge_kernel(DiffSide a, DiffSide b,
                                                                const uint8_t *__restrict__ arena, DeltaScratch w) {
    __shared__ unsigned long long best[2];
    const uint64_t total = *w.n_tiles, n_runs = *w.n_runs;
    for (uint64_t T = blockIdx.x; T < total; T += gridDim.x) {
        const uint64_t k = diff_span_at(w.tstart, b.n - 1, T);  // the last run that starts at or below T has tiles
        const DeltaRegion g = region_of(w, k, n_runs, a.size, b.size);
        const uint64_t t = T - w.tstart[k];
        if (threadIdx.x == 0) best[0] = ~0ull, best[1] = 0;
        __syncthreads();
        uint64_t x0, x1, s0, s1, first, last;
        const uint64_t e_now = peek(w.fwd + k), m_now = peek(w.bwd + k);
        delta_fwd_tile(g, t, &x0, &x1);
        if (x0 - g.l < e_now &&
            delta_segment(x0, x1, threadIdx.x, false, g.l, g.l + delta_fwd_cap(g, a.size), &s0, &s1)) {
            seg_compare(a, b, arena, s0, s1, g.dl, &first, &last);
            if (first != ~0ull) atomicMin(&best[0], (unsigned long long)(first - g.l));
        }
        delta_bwd_tile(g, t, &x0, &x1);
        if (x1 > m_now && delta_segment(x0, x1, threadIdx.x, true, delta_bwd_floor(g, a.size), g.r, &s0, &s1)) {
            seg_compare(a, b, arena, s0, s1, g.dr, &first, &last);
            if (last != ~0ull) atomicMax(&best[1], (unsigned long long)(last + 1));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (best[0] < e_now) atomicMin(w.fwd + k, best[0]);
            if (best[1] > m_now) atomicMax(w.bwd + k, best[1]);
        }
        __syncthreads();
    }
}

// ---- ops ---------------------------------------------------------------------------------
// The ops run k opens, as bits: a region's prefix COPY, LITERAL and suffix COPY
// (delta_region_heads), a COPY run's bit 0.  *e, *f: a region's clipped edges.
__device__ __forceinline__ uint32_t run_heads(const DeltaScratch &w, uint64_t k, uint64_t n_runs, uint64_t size_a,
                                              uint64_t size_b, DeltaRegion *g, uint64_t *e, uint64_t *f) {
    *g = region_of(w, k, n_runs, size_a, size_b);
    if (w.rd[k] == kDeltaNone) {
        const uint64_t len = g->r - g->l;
        *e = w.fwd[k];
        *f = delta_clip(len, *e, g->r - w.bwd[k]);
        return delta_region_heads(len, *e, *f, g->dl, g->dr, k > 0);
    }
    *e = *f = 0;
    if (k == 0 || w.rd[k - 1] != kDeltaNone) return 1;  // the first op, or after a COPY run of another diagonal
    const DeltaRegion p = region_of(w, k - 1, n_runs, size_a, size_b);
    const uint64_t len = p.r - p.l, pe = w.fwd[k - 1], pf = delta_clip(len, pe, p.r - w.bwd[k - 1]);
    return delta_copy_head_after_region(len, pe, pf, p.dl, w.rd[k]) ? 1 : 0;
}

__global__ __launch_bounds__(kDlThreads) void delta_count_kernel(uint64_t size_a, uint64_t size_b, uint64_t nb,
                                                                 DeltaScratch w) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_runs = *w.n_runs;
    uint64_t literal = 0;
    if (k < nb) {
        uint32_t heads = 0;
        if (k < n_runs) {
            DeltaRegion g;
            uint64_t e, f;
            heads = run_heads(w, k, n_runs, size_a, size_b, &g, &e, &f);
            if (w.rd[k] == kDeltaNone) literal = g.r - g.l - e - f;
        }
        w.hcount[k] = __popc(heads);
    }
    wave_add(w.acc, literal);
}

__global__ __launch_bounds__(kDlThreads) void delta_head_kernel(uint64_t size_a, uint64_t size_b, DeltaScratch w) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_runs = *w.n_runs;
    if (k >= n_runs) return;
    DeltaRegion g;
    uint64_t e, f;
    const uint32_t heads = run_heads(w, k, n_runs, size_a, size_b, &g, &e, &f);
    uint64_t at = w.hcount[k];
    if (w.rd[k] != kDeltaNone) {
        if (heads) w.hb[at] = g.l, w.ha[at] = delta_a_index(g.l, w.rd[k]);
        return;
    }
    if (heads & 1) w.hb[at] = g.l, w.ha[at] = delta_a_index(g.l, g.dl), ++at;
    if (heads & 2) w.hb[at] = g.l + e, w.ha[at] = ~0ull, ++at;
    if (heads & 4) w.hb[at] = g.r - f, w.ha[at] = delta_a_index(g.r - f, g.dr);
}

// An op ends where the next begins.  Nothing is written above cap.
__global__ __launch_bounds__(kDlThreads) void delta_emit_kernel(uint64_t size_b, DeltaScratch w, DeltaOp *ops,
                                                                uint64_t cap, unsigned long long *h_out) {
    const uint64_t n = *w.n_ops;
    const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 == 0) {
        h_out[0] = n;
        h_out[1] = size_b - w.acc[0];
        h_out[2] = w.acc[0];
        h_out[3] = w.acc[1];
        h_out[4] = w.acc[2];
        h_out[5] = w.acc[3];
    }
    if (n > cap) return;
    for (uint64_t i = i0; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        ops[i] = DeltaOp{w.hb[i], (i + 1 < n ? w.hb[i + 1] : size_b) - w.hb[i], w.ha[i]};
}

}  // namespace

hipError_t launch_files_delta(const DiffSide &a, const DiffSide &b, uint64_t arena, bool tables_only,
                              const DeltaScratch &w, DeltaOp *d_ops, uint64_t cap, unsigned long long *h_out,
                              hipStream_t s) {
    const uint64_t nb = b.n;
    hipError_t e = hipMemsetAsync(w.acc, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    // 1. A's (slot, span) pairs, sorted: stable, so each slot's group ascends in offset.
    delta_key_kernel<<<grid_of(a.n), kDlThreads, 0, s>>>(a.slot, a.n, w.key_in, w.idx_in);
    size_t sort_bytes = w.sort_bytes;
    if ((e = launch_retain_sort(w.sort_tmp, &sort_bytes, w.key_in, w.key, w.idx_in, w.idx, a.n, 32, s)) != hipSuccess)
        return e;
    // 2. Anchors.  3. Runs and regions.
    delta_match_kernel<<<grid_of(nb), kDlThreads, 0, s>>>(a, b, w.key, w.idx, w.diag, w.acc);
    delta_flag_kernel<<<grid_of(nb), kDlThreads, 0, s>>>(b, w.diag, w.rflag);
    if ((e = launch_store_scan(w.rflag, nb, w.bs_r, nullptr, s)) != hipSuccess) return e;
    delta_run_kernel<<<grid_of(nb), kDlThreads, 0, s>>>(b, w.diag, w);
    delta_region_kernel<<<grid_of(nb), kDlThreads, 0, s>>>(a.size, b.size, nb, tables_only, w);
    // 4. Edges.
    if (!tables_only) {
        if ((e = launch_store_scan(w.tstart, nb, w.bs_t, nullptr, s)) != hipSuccess) return e;
        const unsigned grid = (unsigned)(w.max_tiles < kDlMaxBlocks ? w.max_tiles : kDlMaxBlocks);
        delta_edge_kernel<<<grid, kDlThreads, 0, s>>>(a, b, reinterpret_cast<const uint8_t *>(arena), w);
    }
    // 5. Clip, flag, scan, emit.
    delta_count_kernel<<<grid_of(nb), kDlThreads, 0, s>>>(a.size, b.size, nb, w);
    if ((e = launch_store_scan(w.hcount, nb, w.bs_h, nullptr, s)) != hipSuccess) return e;
    delta_head_kernel<<<grid_of(nb), kDlThreads, 0, s>>>(a.size, b.size, w);
    const uint64_t most = 3 * nb < cap ? 3 * nb : cap;
    const uint64_t blocks = (most + kDlThreads - 1) / kDlThreads;
    delta_emit_kernel<<<(unsigned)(blocks < 1 ? 1 : blocks < kDlMaxBlocks ? blocks : kDlMaxBlocks), kDlThreads, 0, s>>>(
        b.size, w, d_ops, cap, h_out);
    return hipGetLastError();
}

}  // namespace cdc
