// store.hip -- device chunk store: the dedup index (index.hip) plus an HBM
// arena holding the bytes of each first-seen chunk.
//
// Mirrors the reference's key -> data Database (src/system/database.rs:10-36,
// 74-87: insert / get / get_multi / contains, first insert wins),
// ChunkStorage::retrieve (src/system/storage.rs:141-157) and
// FileSystem::read_file_complete (src/system/mod.rs:149-160: look up every
// span's hash, concatenate).
//
// Layout: the index's table with one more per-slot array, loc[slot] = arena
// offset of the digest's bytes.  Stored chunks start at 16-byte multiples; the
// new chunks of a batch are laid out in chunk order (exclusive scan of the
// padded lengths over the index's first-occurrence flags).
//
// put and get move bytes with the same kernel: a list of pieces {src, dst,
// len} is cut into tiles of kStoreTile destination bytes (tile k of a piece
// covers the aligned window [dst & ~15, ...) + k * kStoreTile), the tile
// counts are scanned, and each wave finds its piece by binary search over
// that scan.  A 3 MiB chunk and 20 000 seven-byte chunks both spread over the
// machine.  Inside a tile every lane owns 16-byte slots aligned on the
// DESTINATION: a slot that lies wholly inside the piece is one 16-byte store
// fed by aligned 16-byte loads (two when the source is misaligned against the
// destination, funnel-shifted in registers); the ragged head and tail slots
// are byte copies.  No load leaves the aligned 16-byte blocks that hold source
// bytes, no store touches a byte outside the destination.
#include "store.hpp"

namespace cdc {
namespace {

constexpr int kStThreads = 256;
constexpr int kStWaves = kStThreads / 64;
constexpr int kScanPerThread = (int)(kScanBlockItems / kStThreads);
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

__device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) {
    const uint64_t c = a + b;
    return c < a ? ~0ull : c;
}

// Exclusive scan of one value per thread over the block (kStThreads threads);
// total = the block's sum.  lds: kStWaves entries.
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t *lds, uint64_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const uint64_t o = __shfl_up(inc, k);
        if (lane >= k) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kStWaves; ++w) {
        const uint64_t x = lds[w];
        if (w < wave) base += x;
        tot += x;
    }
    __syncthreads();  // lds may be written again
    total = tot;
    return base + inc - v;
}

// ---- exclusive scan of n u64, three passes ----------------------------------
__global__ __launch_bounds__(kStThreads) void scan_reduce_kernel(const uint64_t *__restrict__ v, uint64_t n,
                                                                 uint64_t *block_sums) {
    __shared__ uint64_t lds[kStWaves];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanBlockItems + (uint64_t)threadIdx.x * kScanPerThread;
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k)
        if (i0 + k < n) sum += v[i0 + k];
    uint64_t total;
    (void)block_excl_scan(sum, lds, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// One block: exclusive scan of block_sums[0, nb) in place; the grand total goes
// to block_sums[nb] and to *total_out (nullable).
__global__ __launch_bounds__(kStThreads) void scan_sums_kernel(uint64_t *block_sums, uint64_t nb,
                                                               unsigned long long *total_out) {
    __shared__ uint64_t lds[kStWaves];
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += kStThreads) {
        const uint64_t i = b0 + threadIdx.x;
        const uint64_t x = i < nb ? block_sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_excl_scan(x, lds, total);
        if (i < nb) block_sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        block_sums[nb] = carry;
        if (total_out) *total_out = carry;
    }
}

__global__ __launch_bounds__(kStThreads) void scan_apply_kernel(uint64_t *v, uint64_t n,
                                                                const uint64_t *__restrict__ block_sums) {
    __shared__ uint64_t lds[kStWaves];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanBlockItems + (uint64_t)threadIdx.x * kScanPerThread;
    uint64_t x[kScanPerThread];
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
        x[k] = i0 + k < n ? v[i0 + k] : 0;
        sum += x[k];
    }
    uint64_t total;
    uint64_t run = block_sums[blockIdx.x] + block_excl_scan(sum, lds, total);
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
        if (i0 + k < n) v[i0 + k] = run;
        run += x[k];
    }
}

// v[0, n) becomes its exclusive scan; block_sums: store_scan_blocks(n) + 1 entries.
void scan_exclusive(uint64_t *v, uint64_t n, uint64_t *block_sums, unsigned long long *total_out, hipStream_t s) {
    const uint64_t nb = store_scan_blocks(n);
    scan_reduce_kernel<<<(unsigned)nb, kStThreads, 0, s>>>(v, n, block_sums);
    scan_sums_kernel<<<1, kStThreads, 0, s>>>(block_sums, nb, total_out);
    scan_apply_kernel<<<(unsigned)nb, kStThreads, 0, s>>>(v, n, block_sums);
}

// ---- put ---------------------------------------------------------------------
__global__ __launch_bounds__(kStThreads) void precheck_kernel(const cdc_chunk_pod *__restrict__ chunks, uint64_t n,
                                                              const uint64_t *__restrict__ streams,
                                                              const uint64_t *__restrict__ lens,
                                                              const uint64_t *__restrict__ first, uint64_t ns,
                                                              StorePiece *pieces, unsigned long long *acc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t bad = 0, pad = 0, tiles = 0;
    if (i < n) {
        uint64_t lo = 0, hi = ns;  // last stream j with first[j] <= i
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (first[mid] <= i) lo = mid;
            else hi = mid;
        }
        const uint64_t off = chunks[i].offset, len = chunks[i].length, L = lens[lo];
        // Inside the buffer, compared without overflow; a length whose padding
        // would wrap 64 bits is no chunk of any buffer.
        const bool ok = off <= L && len <= L - off && len <= ~0ull - (kStoreAlign - 1);
        StorePiece p{0, 0, 0};
        if (ok) {
            p.src = streams[lo] + off;
            p.len = len;
            pad = (len + (kStoreAlign - 1)) & ~(kStoreAlign - 1);
            tiles = (len + (kStoreTile - 1)) / kStoreTile;
        } else {
            bad = 1;
        }
        pieces[i] = p;
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {  // one atomic per wave per counter
        bad += __shfl_xor(bad, k);
        pad = sat_add(pad, __shfl_xor(pad, k));
        tiles += __shfl_xor(tiles, k);
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(&acc[0], (unsigned long long)bad);
        if (pad) {  // every add is one atomic, so a wrap of the 64-bit sum shows in the value it returns
            const unsigned long long old = atomicAdd(&acc[1], (unsigned long long)pad);
            if (old + pad < old) atomicAdd(&acc[3], 1ull);
        }
        if (tiles) atomicAdd(&acc[2], (unsigned long long)tiles);  // <= the padded sum: wraps only if that did
    }
}

__global__ __launch_bounds__(kStThreads) void padded_new_kernel(const StorePiece *__restrict__ pieces,
                                                                const uint8_t *__restrict__ is_new, uint64_t n,
                                                                uint64_t *val) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    val[i] = is_new[i] ? (pieces[i].len + (kStoreAlign - 1)) & ~(kStoreAlign - 1) : 0;
}

__global__ __launch_bounds__(kStThreads) void place_kernel(uint64_t arena, uint64_t arena_used, uint64_t *loc,
                                                           const uint32_t *__restrict__ slot_of,
                                                           const uint8_t *__restrict__ is_new,
                                                           const uint64_t *__restrict__ val, StorePiece *pieces,
                                                           uint64_t n, uint64_t *tiles) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t t = 0;
    const uint32_t s = slot_of[i];
    if (is_new[i] && s != kNoSlot) {
        const uint64_t at = arena_used + val[i];
        loc[s] = at;
        pieces[i].dst = arena + at;  // 16-aligned: tiles start at the piece
        t = (pieces[i].len + (kStoreTile - 1)) / kStoreTile;
    } else {
        pieces[i].len = 0;
    }
    tiles[i] = t;
}

// ---- get / contains ------------------------------------------------------------
__device__ __forceinline__ bool same_digest(const uint8_t *a, const uint8_t *b) {
    const uint4 *x = reinterpret_cast<const uint4 *>(a), *y = reinterpret_cast<const uint4 *>(b);
    const uint4 x0 = x[0], x1 = x[1], y0 = y[0], y1 = y[1];
    return x0.x == y0.x && x0.y == y0.y && x0.z == y0.z && x0.w == y0.w &&
           x1.x == y1.x && x1.y == y1.y && x1.z == y1.z && x1.w == y1.w;
}

__global__ __launch_bounds__(kStThreads) void lookup_kernel(IndexTable t, const uint64_t *__restrict__ loc,
                                                            uint64_t arena, const uint8_t *__restrict__ digests,
                                                            uint64_t n, StorePiece *pieces, uint8_t *found,
                                                            unsigned long long *res) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t missing = 0;
    if (i < n) {
        const uint8_t *d = digests + 32 * i;
        const uint2 w = *reinterpret_cast<const uint2 *>(d);
        const uint64_t key = (((uint64_t)w.y << 32) | w.x) | 1ull;  // index.hip key_of
        const uint64_t mask = t.slots - 1;
        uint64_t s = (key >> 1) & mask;
        StorePiece p{0, 0, 0};
        bool hit = false;
        for (uint64_t probe = 0; probe < t.slots; ++probe, s = (s + 1) & mask) {
            const uint64_t cur = t.tag[s];
            if (cur == 0) break;
            // A tag match of another digest (64-bit key collision, placed further
            // along by the index's serial pass) is not the end of the probe.
            if (cur == key && same_digest(t.digest + 32 * s, d)) {
                p.src = arena + loc[s];
                p.len = t.length[s];
                hit = true;
                break;
            }
        }
        pieces[i] = p;
        if (found) found[i] = hit ? 1 : 0;
        missing = hit ? 0 : 1;
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) missing += __shfl_xor(missing, k);
    if ((threadIdx.x & 63) == 0 && missing) atomicAdd(&res[0], (unsigned long long)missing);
}

__global__ __launch_bounds__(kStThreads) void lengths_kernel(const StorePiece *__restrict__ pieces, uint64_t n,
                                                             uint64_t *val) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) val[i] = pieces[i].len;
}

__global__ __launch_bounds__(kStThreads) void dest_kernel(StorePiece *pieces, uint64_t n, uint64_t d_out,
                                                          const uint64_t *__restrict__ val, uint64_t *tiles) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t dst = d_out + val[i], len = pieces[i].len;
    pieces[i].dst = dst;
    tiles[i] = len ? ((dst & (kStoreAlign - 1)) + len + (kStoreTile - 1)) / kStoreTile : 0;
}

__global__ __launch_bounds__(kStThreads) void spans_kernel(const StorePiece *__restrict__ pieces, uint64_t n,
                                                           uint64_t d_out, cdc_chunk_pod *spans) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) spans[i] = cdc_chunk_pod{pieces[i].dst - d_out, pieces[i].len};
}

// ---- the copy ------------------------------------------------------------------
// Addresses arrive as integers: name the global address space, or the loads
// and stores become flat ones.
#define ST_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef ST_GLOBAL const u32x4 *gload16_t;
typedef ST_GLOBAL u32x4 *gstore16_t;
typedef ST_GLOBAL const uint8_t *gload1_t;
typedef ST_GLOBAL uint8_t *gstore1_t;

// 16 source bytes at address sa, whose misalignment r = sa & 15 is the same for
// the whole wave: aligned 16-byte loads, the shift taken out in registers.
template <int Q>
__device__ __forceinline__ u32x4 funnel(const u32x4 a, const u32x4 b, uint32_t sh) {
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    u32x4 o;
    o.x = __builtin_amdgcn_alignbyte(w[Q + 1], w[Q + 0], sh);
    o.y = __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], sh);
    o.z = __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], sh);
    o.w = __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], sh);
    return o;
}

__device__ __forceinline__ u32x4 load16(uint64_t sa, uint32_t r) {
    if (r == 0) return *reinterpret_cast<gload16_t>(sa);
    gload16_t base = reinterpret_cast<gload16_t>(sa - r);
    const u32x4 a = base[0], b = base[1];  // both blocks hold bytes of [sa, sa + 16)
    const uint32_t sh = r & 3;
    switch (r >> 2) {
        case 0: return funnel<0>(a, b, sh);
        case 1: return funnel<1>(a, b, sh);
        case 2: return funnel<2>(a, b, sh);
        default: return funnel<3>(a, b, sh);
    }
}

// Wave w copies tile w - tstart[p] of piece p, p = the last piece with
// tstart[p] <= w.  total_ptr (nullable) overrides `total` with a device value.
__global__ __launch_bounds__(kStThreads) void copy_kernel(const StorePiece *__restrict__ pieces,
                                                          const uint64_t *__restrict__ tstart, uint64_t n,
                                                          uint64_t total, const uint64_t *total_ptr) {
    if (total_ptr) total = *total_ptr;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kStWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * kStWaves;
    for (uint64_t w = wave0; w < total; w += nwaves) {
        uint64_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (tstart[mid] <= w) lo = mid;
            else hi = mid;
        }
        const StorePiece p = pieces[lo];
        const uint64_t end = p.dst + p.len;
        const uint64_t tb = (p.dst & ~(kStoreAlign - 1)) + (w - tstart[lo]) * kStoreTile;
        const uint64_t te = tb + kStoreTile < end ? tb + kStoreTile : end;
        const uint64_t shift = p.src - p.dst;  // source address = destination address + shift
        const uint32_t r = (uint32_t)shift & 15u;
        for (uint64_t a = tb + lane * 16; a < te; a += 64 * 16) {
            if (a >= p.dst && a + 16 <= end) {
                *reinterpret_cast<gstore16_t>(a) = load16(a + shift, r);
            } else {  // ragged head or tail of the piece
                const uint64_t b0 = a > p.dst ? a : p.dst, b1 = a + 16 < end ? a + 16 : end;
                for (uint64_t b = b0; b < b1; ++b)
                    *reinterpret_cast<gstore1_t>(b) = *reinterpret_cast<gload1_t>(b + shift);
            }
        }
    }
}

constexpr uint64_t kMaxCopyBlocks = 1u << 20;  // waves past this stride over the tiles

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kStThreads - 1) / kStThreads); }

inline unsigned copy_grid(uint64_t tiles) {
    const uint64_t blocks = (tiles + kStWaves - 1) / kStWaves;
    return (unsigned)(blocks < kMaxCopyBlocks ? blocks : kMaxCopyBlocks);
}

}  // namespace

hipError_t launch_store_precheck(const void *d_chunks, uint64_t n, const uint64_t *d_streams,
                                 const uint64_t *d_lens, const uint64_t *d_first, uint64_t n_streams,
                                 StorePiece *pieces, unsigned long long *d_acc, hipStream_t s) {
    if (!n) return hipSuccess;
    precheck_kernel<<<grid_of(n), kStThreads, 0, s>>>(reinterpret_cast<const cdc_chunk_pod *>(d_chunks), n,
                                                      d_streams, d_lens, d_first, n_streams, pieces, d_acc);
    return hipGetLastError();
}

hipError_t launch_store_compact(uint8_t *arena, uint64_t arena_used, uint64_t *loc, const uint32_t *d_slot_of,
                                const uint8_t *d_new, StorePiece *pieces, uint64_t n, uint64_t *val,
                                uint64_t *tstart, uint64_t *block_sums, uint64_t max_tiles,
                                unsigned long long *d_taken, hipStream_t s) {
    if (!n) return hipSuccess;
    padded_new_kernel<<<grid_of(n), kStThreads, 0, s>>>(pieces, d_new, n, val);
    scan_exclusive(val, n, block_sums, d_taken, s);
    place_kernel<<<grid_of(n), kStThreads, 0, s>>>((uint64_t)(uintptr_t)arena, arena_used, loc, d_slot_of, d_new,
                                                   val, pieces, n, tstart);
    scan_exclusive(tstart, n, block_sums, nullptr, s);
    if (max_tiles)  // the tile count of the new chunks is block_sums[blocks], on the device
        copy_kernel<<<copy_grid(max_tiles), kStThreads, 0, s>>>(pieces, tstart, n, 0,
                                                                block_sums + store_scan_blocks(n));
    return hipGetLastError();
}

hipError_t launch_store_lookup(const IndexTable &t, const uint64_t *loc, const uint8_t *arena,
                               const uint8_t *d_digests, uint64_t n, StorePiece *pieces, uint8_t *found,
                               unsigned long long *d_res, hipStream_t s) {
    if (!n) return hipSuccess;
    lookup_kernel<<<grid_of(n), kStThreads, 0, s>>>(t, loc, (uint64_t)(uintptr_t)arena, d_digests, n, pieces,
                                                    found, d_res);
    return hipGetLastError();
}

hipError_t launch_store_plan_get(StorePiece *pieces, uint64_t n, uint64_t d_out, uint64_t *val, uint64_t *tstart,
                                 uint64_t *block_sums, unsigned long long *d_res, hipStream_t s) {
    if (!n) return hipSuccess;
    lengths_kernel<<<grid_of(n), kStThreads, 0, s>>>(pieces, n, val);
    scan_exclusive(val, n, block_sums, d_res + 1, s);
    dest_kernel<<<grid_of(n), kStThreads, 0, s>>>(pieces, n, d_out, val, tstart);
    scan_exclusive(tstart, n, block_sums, d_res + 2, s);
    return hipGetLastError();
}

hipError_t launch_store_scan(uint64_t *v, uint64_t n, uint64_t *block_sums, unsigned long long *total_out,
                             hipStream_t s) {
    if (!n) return hipSuccess;
    scan_exclusive(v, n, block_sums, total_out, s);
    return hipGetLastError();
}

hipError_t launch_store_copy(const StorePiece *pieces, const uint64_t *tstart, uint64_t n, uint64_t max_tiles,
                             const uint64_t *d_total, hipStream_t s) {
    if (!n || !max_tiles) return hipSuccess;
    copy_kernel<<<copy_grid(max_tiles), kStThreads, 0, s>>>(pieces, tstart, n, 0, d_total);
    return hipGetLastError();
}

hipError_t launch_store_gather(const StorePiece *pieces, const uint64_t *tstart, uint64_t n, uint64_t tiles,
                               uint64_t d_out, void *d_spans, hipStream_t s) {
    if (!n) return hipSuccess;
    if (tiles) copy_kernel<<<copy_grid(tiles), kStThreads, 0, s>>>(pieces, tstart, n, tiles, nullptr);
    if (d_spans)
        spans_kernel<<<grid_of(n), kStThreads, 0, s>>>(pieces, n, d_out, reinterpret_cast<cdc_chunk_pod *>(d_spans));
    return hipGetLastError();
}

}  // namespace cdc
