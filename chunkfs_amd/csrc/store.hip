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
//
// Scrub stage (the reference's Scrub hook, src/system/scrub.rs, and the
// DataContainer that is a chunk or a list of target keys, storage.rs:12-21):
// with a target store attached a slot also has a kind and, for a target, a run
// of resolved keys {target slot, byte offset inside the container}.  The scrub
// lists the chunk-kind containers with the scan above, the target's put takes
// their bytes (COPY) or their re-chunked sub-chunks (RECHUNK) straight from this
// arena, and a marking kernel writes the key runs; get then expands a digest
// into one piece per key and feeds the same copy kernel.
//
// Bench fixture (the reference's CDCFixture, src/bench/mod.rs:218-275): verify
// runs the copy's piece list through compare_kernel -- the same tiles and loads,
// a comparison in place of the store -- and the size distribution is a
// max-reduce, a wave-aggregated histogram and a compaction over the slots.
//
// Retain / collect (not in the reference; DESIGN.md "Removal and collection"):
// from per-slot reference counts the survivors are listed, ordered by arena
// offset (rocPRIM's radix sort, bookkeeping only) and given new offsets by a
// scan of their padded lengths; one thread plans move groups over those scans;
// the bytes slide down in place through the copy kernel, a group either straight
// to its new place or through a bounce buffer; the survivors are inserted into
// a second, zeroed table with the unchanged index insert.
#include <rocprim/device/device_radix_sort.hpp>

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

// ---- the compare -----------------------------------------------------------------
// The same value in every lane, provably so for the compiler.
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// Index of the first byte in which two 16-byte blocks differ; 16 when equal.
__device__ __forceinline__ uint32_t first_diff16(const u32x4 x, const u32x4 y) {
    const uint32_t d0 = x.x ^ y.x, d1 = x.y ^ y.y, d2 = x.z ^ y.z, d3 = x.w ^ y.w;
    if (d0) return (uint32_t)__builtin_ctz(d0) >> 3;
    if (d1) return 4u + ((uint32_t)__builtin_ctz(d1) >> 3);
    if (d2) return 8u + ((uint32_t)__builtin_ctz(d2) >> 3);
    if (d3) return 12u + ((uint32_t)__builtin_ctz(d3) >> 3);
    return 16u;
}

// copy_kernel with the store replaced by a comparison: piece p says that the
// bytes [dst, dst + len) -- the caller's dataset -- should equal [src, src +
// len) -- the arena.  Same mapping (wave per tile, tiles aligned on dst), same
// loads: the dst side is read with aligned 16-byte loads strictly inside the
// piece, the src side through load16, ragged heads and tails bytewise; nothing
// is written but *diff.  A lane keeps the address of its first differing byte,
// the wave reduces to the minimum, and one atomicMin per differing wave leaves
// in *diff the smallest differing offset from `base` (preset to ~0).  A tile
// that starts at or past the minimum found so far cannot lower it and is
// skipped; that read is a plain load and changes no result.
__global__ __launch_bounds__(kStThreads) void compare_kernel(const StorePiece *__restrict__ pieces,
                                                             const uint64_t *__restrict__ tstart, uint64_t n,
                                                             const uint64_t *total_ptr, uint64_t base,
                                                             unsigned long long *diff) {
    const uint64_t total = *total_ptr;
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
        const uint64_t found = uniform64(*reinterpret_cast<const volatile unsigned long long *>(diff));
        if ((tb > p.dst ? tb : p.dst) - base >= found) continue;  // the same decision in every lane
        const uint64_t shift = p.src - p.dst;  // arena address = dataset address + shift
        const uint32_t r = (uint32_t)shift & 15u;
        uint64_t at = ~0ull;
        for (uint64_t a = tb + lane * 16; a < te; a += 64 * 16) {
            if (a >= p.dst && a + 16 <= end) {
                const uint32_t k = first_diff16(*reinterpret_cast<gload16_t>(a), load16(a + shift, r));
                if (k < 16u && a + k < at) at = a + k;
            } else {  // ragged head or tail of the piece
                const uint64_t b0 = a > p.dst ? a : p.dst, b1 = a + 16 < end ? a + 16 : end;
                for (uint64_t b = b0; b < b1; ++b)
                    if (*reinterpret_cast<gload1_t>(b) != *reinterpret_cast<gload1_t>(b + shift)) {
                        if (b < at) at = b;
                        break;
                    }
            }
        }
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const uint64_t o = __shfl_xor(at, k);
            at = o < at ? o : at;
        }
        if (lane == 0 && at != ~0ull) atomicMin(diff, (unsigned long long)(at - base));
    }
}

// ---- the difference mask -----------------------------------------------------------
// One bit per byte of a 16-byte block: set where x and y differ.
__device__ __forceinline__ uint32_t diff_bits4(uint32_t d) {
    uint32_t t = d | (d >> 4);
    t |= t >> 2;
    t |= t >> 1;
    t &= 0x01010101u;  // bit 0 of each byte: the byte is not zero
    return (t | (t >> 7) | (t >> 14) | (t >> 21)) & 0xFu;
}
__device__ __forceinline__ uint32_t diff_bits16(const u32x4 x, const u32x4 y) {
    return diff_bits4(x.x ^ y.x) | (diff_bits4(x.y ^ y.y) << 4) | (diff_bits4(x.z ^ y.z) << 8) |
           (diff_bits4(x.w ^ y.w) << 12);
}

// compare_kernel with the first-difference minimum replaced by one bit per byte
// (cdc_files_diff_device): piece p says that the bytes [dst, dst + len) and
// [src, src + len) are the two sides.  Same mapping (wave per tile, tiles
// aligned on dst), same loads: dst with aligned 16-byte loads strictly inside
// the piece, src through load16, ragged heads and tails bytewise.  Tile w owns
// the 64 words mask[64 w ..]: bit b of the tile is the byte at its address tb +
// b, set when the two sides differ there; the bits outside the piece are
// written as zero.  Four lanes share a word: their 16-bit parts meet by shuffle.
__global__ __launch_bounds__(kStThreads) void diff_mask_kernel(const StorePiece *__restrict__ pieces,
                                                               const uint64_t *__restrict__ tstart, uint64_t n,
                                                               const uint64_t *total_ptr, uint64_t *mask) {
    const uint64_t total = *total_ptr;
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
        const uint64_t shift = p.src - p.dst;  // A's address = B's address + shift
        const uint32_t r = (uint32_t)shift & 15u;
#pragma unroll
        for (uint32_t it = 0; it < kStoreTile / (64 * 16); ++it) {
            const uint64_t a = tb + (uint64_t)it * (64 * 16) + lane * 16;
            uint32_t bits = 0;
            if (a < te) {
                if (a >= p.dst && a + 16 <= end) {
                    bits = diff_bits16(*reinterpret_cast<gload16_t>(a), load16(a + shift, r));
                } else {  // ragged head or tail of the piece
                    const uint64_t b0 = a > p.dst ? a : p.dst, b1 = a + 16 < end ? a + 16 : end;
                    for (uint64_t b = b0; b < b1; ++b)
                        if (*reinterpret_cast<gload1_t>(b) != *reinterpret_cast<gload1_t>(b + shift))
                            bits |= 1u << (uint32_t)(b - a);
                }
            }
            uint64_t v = (uint64_t)bits << (16 * (lane & 3));
            v |= __shfl_xor(v, 1);
            v |= __shfl_xor(v, 2);
            if ((lane & 3) == 0) mask[w * 64 + it * 16 + (lane >> 2)] = v;
        }
    }
}

// ---- scrub stage -----------------------------------------------------------------
// A slot holds a container once a chunk has been recorded as its first insert.
__device__ __forceinline__ bool occupied(const IndexTable &t, uint64_t s) {
    return t.tag[s] != 0 && t.owner[s] != ~0ull;
}

// ---- size distribution -----------------------------------------------------------
// *max_len = the longest container (preset to 0): it sizes the bins.
__global__ __launch_bounds__(kStThreads) void dist_max_kernel(IndexTable t, unsigned long long *max_len) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t len = s < t.slots && occupied(t, s) ? t.length[s] : 0;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const uint64_t o = __shfl_xor(len, k);
        len = o > len ? o : len;
    }
    if ((threadIdx.x & 63) == 0 && len) atomicMax(max_len, (unsigned long long)len);
}

// bins[length / adjustment] += 1 per occupied slot.  The wave aggregates first:
// the lanes that share the leader's bin retire together with one atomic, so a
// store of equal-length containers (FSChunker) costs one atomic per wave.
__global__ __launch_bounds__(kStThreads) void dist_hist_kernel(IndexTable t, uint64_t adjustment, uint32_t *bins) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool todo = s < t.slots && occupied(t, s);
    const uint64_t bin = todo ? t.length[s] / adjustment : 0;
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long left = __ballot(todo);
    while (left) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(left);
        const uint64_t lead_bin = __shfl(bin, (int)leader);
        const bool mine = todo && bin == lead_bin;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&bins[lead_bin], (uint32_t)__popcll(same));
        if (mine) todo = false;
        left &= ~same;
    }
}

__global__ __launch_bounds__(kStThreads) void dist_flag_bins_kernel(const uint32_t *__restrict__ bins, uint64_t nb,
                                                                    uint64_t *val) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nb) val[b] = bins[b] ? 1 : 0;
}

// val = exclusive scan of the flags: the non-empty bins in ascending size order.
__global__ __launch_bounds__(kStThreads) void dist_emit_kernel(const uint32_t *__restrict__ bins, uint64_t nb,
                                                               const uint64_t *__restrict__ val, uint64_t adjustment,
                                                               uint64_t *sizes, uint32_t *counts) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb || !bins[b]) return;
    sizes[val[b]] = b * adjustment;
    counts[val[b]] = bins[b];
}

__global__ __launch_bounds__(kStThreads) void scrub_flag_kernel(IndexTable t, const uint8_t *__restrict__ kind,
                                                                int want_kind, uint64_t *val) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= t.slots) return;
    val[s] = occupied(t, s) && (want_kind < 0 || kind[s] == want_kind) ? 1 : 0;
}

__global__ __launch_bounds__(kStThreads) void scrub_list_kernel(IndexTable t, const uint8_t *__restrict__ kind,
                                                                const uint64_t *__restrict__ loc,
                                                                const uint64_t *__restrict__ val,
                                                                cdc_chunk_pod *chunks, uint8_t *digests,
                                                                uint32_t *slot_of, unsigned long long *bytes) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t len = 0;
    if (s < t.slots && occupied(t, s) && kind[s] == 0) {
        const uint64_t j = val[s];
        len = t.length[s];
        chunks[j] = cdc_chunk_pod{loc[s], len};
        const uint4 *src = reinterpret_cast<const uint4 *>(t.digest + 32 * s);
        uint4 *dst = reinterpret_cast<uint4 *>(digests + 32 * j);
        dst[0] = src[0];
        dst[1] = src[1];
        slot_of[j] = (uint32_t)s;
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) len += __shfl_xor(len, k);
    if ((threadIdx.x & 63) == 0 && len) atomicAdd(bytes, (unsigned long long)len);
}

__global__ __launch_bounds__(kStThreads) void scrub_padsum_kernel(const cdc_chunk_pod *__restrict__ chunks,
                                                                  uint64_t n, unsigned long long *sum) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t pad = i < n ? (chunks[i].length + (kStoreAlign - 1)) & ~(kStoreAlign - 1) : 0;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) pad += __shfl_xor(pad, k);
    if ((threadIdx.x & 63) == 0 && pad) atomicAdd(sum, (unsigned long long)pad);
}

// Thread i < nc turns container i into a target; thread i < n writes key i.
__global__ __launch_bounds__(kStThreads) void scrub_mark_kernel(ScrubState w, const uint32_t *__restrict__ c_slot,
                                                                uint64_t nc, const uint64_t *__restrict__ first,
                                                                const cdc_chunk_pod *__restrict__ sub,
                                                                const uint32_t *__restrict__ t_slot, uint64_t n,
                                                                uint64_t key_base) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nc) {
        const uint32_t s = c_slot[i];
        const uint64_t f0 = first ? first[i] : i, f1 = first ? first[i + 1] : i + 1;
        w.kind[s] = 1;
        w.key_first[s] = key_base + f0;
        w.key_count[s] = (uint32_t)(f1 - f0);
    }
    if (i < n) {
        w.key_slot[key_base + i] = t_slot[i];
        w.key_off[key_base + i] = sub ? sub[i].offset : 0;
    }
}

__global__ __launch_bounds__(kStThreads) void lookup_x_kernel(IndexTable t, ScrubView v,
                                                              const uint8_t *__restrict__ digests, uint64_t n,
                                                              uint32_t *slot_of, uint64_t *cnt, uint64_t *val,
                                                              unsigned long long *res) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t missing = 0, targets = 0;
    if (i < n) {
        const uint8_t *d = digests + 32 * i;
        const uint2 w = *reinterpret_cast<const uint2 *>(d);
        const uint64_t key = (((uint64_t)w.y << 32) | w.x) | 1ull;  // index.hip key_of
        const uint64_t mask = t.slots - 1;
        uint64_t s = (key >> 1) & mask;
        uint32_t hit = kNoSlot;
        for (uint64_t probe = 0; probe < t.slots; ++probe, s = (s + 1) & mask) {
            const uint64_t cur = t.tag[s];
            if (cur == 0) break;
            if (cur == key && same_digest(t.digest + 32 * s, d)) {
                hit = (uint32_t)s;
                break;
            }
        }
        slot_of[i] = hit;
        if (hit == kNoSlot) {
            missing = 1;
            cnt[i] = 0;
            val[i] = 0;
        } else {
            targets = v.kind[hit];
            cnt[i] = targets ? v.key_count[hit] : 1;
            val[i] = t.length[hit];
        }
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        missing += __shfl_xor(missing, k);
        targets += __shfl_xor(targets, k);
    }
    if ((threadIdx.x & 63) == 0) {
        if (missing) atomicAdd(&res[0], (unsigned long long)missing);
        if (targets) atomicAdd(&res[3], (unsigned long long)targets);
    }
}

__global__ __launch_bounds__(kStThreads) void pieces_x_kernel(IndexTable t, ScrubView v,
                                                              const uint64_t *__restrict__ loc, uint64_t arena,
                                                              const uint32_t *__restrict__ slot_of,
                                                              const uint64_t *__restrict__ pstart,
                                                              const uint64_t *__restrict__ off, uint64_t n,
                                                              uint64_t d_out, StorePiece *pieces, uint64_t *tiles,
                                                              uint64_t n_pieces) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pieces) return;
    uint64_t a = 0, b = n;  // last digest i with pstart[i] <= p (digests of no pieces share a start)
    while (b - a > 1) {
        const uint64_t mid = (a + b) >> 1;
        if (pstart[mid] <= p) a = mid;
        else b = mid;
    }
    const uint32_t s = slot_of[a];
    StorePiece pc;
    if (v.kind[s]) {
        const uint64_t k = v.key_first[s] + (p - pstart[a]);
        const uint32_t ts = v.key_slot[k];
        pc.src = v.t_arena + v.t_loc[ts];
        pc.dst = d_out + off[a] + v.key_off[k];
        pc.len = v.t_length[ts];
    } else {
        pc.src = arena + loc[s];
        pc.dst = d_out + off[a];
        pc.len = t.length[s];
    }
    pieces[p] = pc;
    tiles[p] = pc.len ? ((pc.dst & (kStoreAlign - 1)) + pc.len + (kStoreTile - 1)) / kStoreTile : 0;
}

__global__ __launch_bounds__(kStThreads) void spans_x_kernel(IndexTable t, const uint32_t *__restrict__ slot_of,
                                                             const uint64_t *__restrict__ off, uint64_t n,
                                                             cdc_chunk_pod *spans) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) spans[i] = cdc_chunk_pod{off[i], t.length[slot_of[i]]};
}

__global__ __launch_bounds__(kStThreads) void iterate_kernel(IndexTable t, ScrubView v,
                                                             const uint64_t *__restrict__ val, uint8_t *digests,
                                                             uint8_t *kinds, uint64_t *lengths, uint64_t *key_first) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= t.slots || !occupied(t, s)) return;
    const uint64_t j = val[s];
    const uint4 *src = reinterpret_cast<const uint4 *>(t.digest + 32 * s);
    uint4 *dst = reinterpret_cast<uint4 *>(digests + 32 * j);
    dst[0] = src[0];
    dst[1] = src[1];
    const uint8_t k = v.kind ? v.kind[s] : 0;
    kinds[j] = k;
    lengths[j] = t.length[s];
    key_first[j] = k ? v.key_count[s] : 0;
}

__global__ __launch_bounds__(kStThreads) void key_counts_kernel(IndexTable t, ScrubView v, uint64_t *val) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= t.slots) return;
    val[s] = occupied(t, s) && v.kind[s] ? v.key_count[s] : 0;
}

// One thread per slot copies its container's keys in a loop (6144 x 32 bytes
// from one lane for a 3 MiB container under 512-byte sub-chunks): enough for
// storage_iterator, not meant for a hot path.
__global__ __launch_bounds__(kStThreads) void keys_kernel(IndexTable t, ScrubView v,
                                                          const uint64_t *__restrict__ val, uint8_t *keys) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= t.slots || !occupied(t, s) || !v.kind[s]) return;
    const uint64_t k0 = v.key_first[s], at = val[s];
    for (uint32_t k = 0; k < v.key_count[s]; ++k) {
        const uint4 *src = reinterpret_cast<const uint4 *>(v.t_digest + 32ull * v.key_slot[k0 + k]);
        uint4 *dst = reinterpret_cast<uint4 *>(keys + 32 * (at + k));
        dst[0] = src[0];
        dst[1] = src[1];
    }
}

// ---- retain / collect --------------------------------------------------------------
// refs[slot] += 1 per digest found (lookup_kernel's probe); res[0] += digests absent.
__global__ __launch_bounds__(kStThreads) void retain_refs_kernel(IndexTable t, const uint8_t *__restrict__ digests,
                                                                 uint64_t n, unsigned long long *refs,
                                                                 unsigned long long *res) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t missing = 0;
    if (i < n) {
        const uint8_t *d = digests + 32 * i;
        const uint2 w = *reinterpret_cast<const uint2 *>(d);
        const uint64_t key = (((uint64_t)w.y << 32) | w.x) | 1ull;  // index.hip key_of
        const uint64_t mask = t.slots - 1;
        uint64_t s = (key >> 1) & mask;
        missing = 1;
        for (uint64_t probe = 0; probe < t.slots; ++probe, s = (s + 1) & mask) {
            const uint64_t cur = t.tag[s];
            if (cur == 0) break;
            if (cur == key && same_digest(t.digest + 32 * s, d)) {
                atomicAdd(&refs[s], 1ull);
                missing = 0;
                break;
            }
        }
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) missing += __shfl_xor(missing, k);
    if ((threadIdx.x & 63) == 0 && missing) atomicAdd(&res[0], (unsigned long long)missing);
}

// val[s] = 1 for the containers that stay (occupied, refs > 0).  acc[0] += sum of
// refs, acc[1] += sum of refs * length, acc[2] += the survivors' bytes, acc[3] =
// their longest padded length: one atomic per wave each.
__global__ __launch_bounds__(kStThreads) void retain_flag_kernel(IndexTable t,
                                                                 const unsigned long long *__restrict__ refs,
                                                                 uint64_t *val, unsigned long long *acc) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t r = 0, rb = 0, ub = 0, mx = 0;
    if (s < t.slots) {
        r = occupied(t, s) ? refs[s] : 0;
        val[s] = r ? 1 : 0;
        if (r) {
            const uint64_t len = t.length[s];
            rb = r * len;
            ub = len;
            mx = (len + (kStoreAlign - 1)) & ~(kStoreAlign - 1);
        }
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        r += __shfl_xor(r, k);
        rb += __shfl_xor(rb, k);
        ub += __shfl_xor(ub, k);
        const uint64_t o = __shfl_xor(mx, k);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        if (r) atomicAdd(&acc[0], (unsigned long long)r);
        if (rb) atomicAdd(&acc[1], (unsigned long long)rb);
        if (ub) atomicAdd(&acc[2], (unsigned long long)ub);
        if (mx) atomicMax(&acc[3], (unsigned long long)mx);
    }
}

// The survivors at their ranks (val = the scanned flags): the sort key is the
// arena offset, a multiple of 16, with bit 0 set for a container that holds
// bytes.  A length-0 container shares its offset with the container stored next
// after it and must stay in front of it, or the gaps would not be monotonic.
__global__ __launch_bounds__(kStThreads) void retain_list_kernel(IndexTable t, const uint64_t *__restrict__ loc,
                                                                 const unsigned long long *__restrict__ refs,
                                                                 const uint64_t *__restrict__ val, uint64_t *key,
                                                                 uint32_t *slot) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= t.slots || !occupied(t, s) || !refs[s]) return;
    const uint64_t j = val[s];
    key[j] = loc[s] | (t.length[s] ? 1ull : 0ull);
    slot[j] = (uint32_t)s;
}

// In arena order: the padded length (scanned into the new offsets afterwards),
// the digest and the {0, length} record the index insert takes.
__global__ __launch_bounds__(kStThreads) void retain_gather_kernel(IndexTable t, const uint32_t *__restrict__ slot,
                                                                   uint64_t m, uint64_t *pad, uint8_t *digests,
                                                                   cdc_chunk_pod *chunks) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t s = slot[i];
    const uint64_t len = t.length[s];
    pad[i] = (len + (kStoreAlign - 1)) & ~(kStoreAlign - 1);
    chunks[i] = cdc_chunk_pod{0, len};
    const uint4 *src = reinterpret_cast<const uint4 *>(t.digest + 32ull * s);
    uint4 *dst = reinterpret_cast<uint4 *>(digests + 32 * i);
    dst[0] = src[0];
    dst[1] = src[1];
}

// Largest b in [a, m] with newloc[b] - newloc[a] <= limit (newloc has m + 1 entries).
__device__ __forceinline__ uint64_t retain_reach(const uint64_t *__restrict__ newloc, uint64_t a, uint64_t m,
                                                 uint64_t limit) {
    uint64_t lo = a, hi = m;
    const uint64_t base = newloc[a];
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (newloc[mid] - base <= limit) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One thread plans the move groups (tests/gc_model.py plan_groups is the same
// rule in Python).  gap[i] = old offset - new offset never decreases along the
// survivors; the leading run with gap 0 stays where it is.  From the first moved
// survivor a on: the direct group [a, bd) is the longest whose bytes fit into
// gap[a], the bounced group [a, bb) the longest whose bytes fit into W.  The
// direct one is taken when it moves at least half of what the bounced one would
// (a bounced byte is copied twice) or reaches the end.  W = max(max_pad,
// min(w_req, bytes to move)) rounded up to 16: at least every padded length, so
// bb > a and the loop advances.  out: [0] groups, [1] direct, [2] bounced, [3]
// bytes moved, [4] groups that did not fit `cap`, [5] W, [6] new offset of the
// first moved byte, [7] newloc[m].
__global__ void retain_plan_kernel(const uint64_t *__restrict__ key, const uint64_t *__restrict__ newloc, uint64_t m,
                                   uint64_t w_req, uint64_t max_pad, RetainGroup *groups, uint64_t cap,
                                   unsigned long long *out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t lo = 0, hi = m;  // first survivor with gap > 0
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((key[mid] & ~(kStoreAlign - 1)) > newloc[mid]) hi = mid;
        else lo = mid + 1;
    }
    uint64_t ng = 0, nd = 0, nb = 0, over = 0;
    const uint64_t first = lo, moved = first < m ? newloc[m] - newloc[first] : 0;
    uint64_t W = w_req < moved ? w_req : moved;
    W = (W + (kStoreAlign - 1)) & ~(kStoreAlign - 1);
    W = W < max_pad ? max_pad : W;
    for (uint64_t a = first; a < m;) {
        const uint64_t gap = (key[a] & ~(kStoreAlign - 1)) - newloc[a];
        const uint64_t bd = retain_reach(newloc, a, m, gap), bb = retain_reach(newloc, a, m, W);
        const uint64_t direct_bytes = newloc[bd] - newloc[a], bounced_bytes = newloc[bb] - newloc[a];
        const bool direct = bd == m || 2 * direct_bytes >= bounced_bytes;
        const uint64_t b = direct ? bd : bb;
        if (b <= a) {  // cannot happen while W >= the longest padded length: stop instead of spinning
            over = ~0ull;
            break;
        }
        if (ng < cap) groups[ng] = RetainGroup{a, b, direct ? direct_bytes : bounced_bytes, direct ? 1ull : 0ull};
        else ++over;
        ++ng;
        if (direct) ++nd;
        else ++nb;
        a = b;
    }
    out[0] = ng;
    out[1] = nd;
    out[2] = nb;
    out[3] = moved;
    out[4] = over;
    out[5] = W;
    out[6] = first < m ? newloc[first] : newloc[m];
    out[7] = newloc[m];
}

// The group of survivor i (groups are consecutive ranges from groups[0].a on);
// ng when it lies in the leading run that does not move.
__device__ __forceinline__ uint64_t retain_group_of(const RetainGroup *__restrict__ groups, uint64_t ng, uint64_t i) {
    if (ng == 0 || i < groups[0].a) return ng;
    uint64_t a = 0, b = ng;
    while (b - a > 1) {
        const uint64_t mid = (a + b) >> 1;
        if (groups[mid].a <= i) a = mid;
        else b = mid;
    }
    return a;
}

// One piece per survivor, padded length (both ends are 16-byte multiples inside
// the arena): to its new offset for a direct group, into the bounce buffer at
// its distance from the group's first byte for a bounced one.
__global__ __launch_bounds__(kStThreads) void retain_pieces_kernel(const uint64_t *__restrict__ key,
                                                                   const uint64_t *__restrict__ newloc, uint64_t m,
                                                                   const RetainGroup *__restrict__ groups, uint64_t ng,
                                                                   uint64_t arena, uint64_t bounce, StorePiece *pieces,
                                                                   uint64_t *tiles) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t g = retain_group_of(groups, ng, i);
    StorePiece p{0, 0, 0};
    if (g < ng) {
        p.src = arena + (key[i] & ~(kStoreAlign - 1));
        p.len = newloc[i + 1] - newloc[i];
        p.dst = groups[g].direct ? arena + newloc[i] : bounce + (newloc[i] - newloc[groups[g].a]);
    }
    pieces[i] = p;
    tiles[i] = (p.len + (kStoreTile - 1)) / kStoreTile;
}

// tstart = the scan of the tile counts over all survivors (m + 1 entries); the
// copy wants each group's scan to start at 0.  Threads [m, m + ng): the group's
// tile count, which the copy reads on the device.
__global__ __launch_bounds__(kStThreads) void retain_rel_kernel(const uint64_t *__restrict__ tstart, uint64_t m,
                                                                const RetainGroup *__restrict__ groups, uint64_t ng,
                                                                uint64_t *trel, uint64_t *gtiles) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m + ng) return;
    if (i >= m) {
        const RetainGroup g = groups[i - m];
        gtiles[i - m] = tstart[g.b] - tstart[g.a];
        return;
    }
    const uint64_t g = retain_group_of(groups, ng, i);
    trel[i] = g < ng ? tstart[i] - tstart[groups[g].a] : 0;
}

// After the insert into the new table: old slot -> new slot (map, preset to
// 0xFFFFFFFF) and the new table's loc entry.
__global__ __launch_bounds__(kStThreads) void retain_scatter_kernel(const uint32_t *__restrict__ old_slot,
                                                                    const uint32_t *__restrict__ new_slot,
                                                                    const uint64_t *__restrict__ newloc, uint64_t m,
                                                                    uint64_t *new_loc, uint32_t *map) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t ns = new_slot[i];
    if (ns == kNoSlot) return;  // the host refuses the call on the insert's counters
    map[old_slot[i]] = ns;
    new_loc[ns] = newloc[i];
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

hipError_t launch_store_compare(const StorePiece *pieces, const uint64_t *tstart, uint64_t n, uint64_t max_tiles,
                                const uint64_t *d_total, uint64_t base, unsigned long long *d_diff, hipStream_t s) {
    if (!n || !max_tiles) return hipSuccess;
    compare_kernel<<<copy_grid(max_tiles), kStThreads, 0, s>>>(pieces, tstart, n, d_total, base, d_diff);
    return hipGetLastError();
}

hipError_t launch_store_diff_mask(const StorePiece *pieces, const uint64_t *tstart, uint64_t n, uint64_t max_tiles,
                                  const uint64_t *d_total, uint64_t *mask, hipStream_t s) {
    if (!n || !max_tiles) return hipSuccess;
    diff_mask_kernel<<<copy_grid(max_tiles), kStThreads, 0, s>>>(pieces, tstart, n, d_total, mask);
    return hipGetLastError();
}

hipError_t launch_store_dist_max(const IndexTable &t, unsigned long long *d_max, hipStream_t s) {
    dist_max_kernel<<<grid_of(t.slots), kStThreads, 0, s>>>(t, d_max);
    return hipGetLastError();
}

hipError_t launch_store_dist_bins(const IndexTable &t, uint64_t adjustment, uint32_t *bins, uint64_t n_bins,
                                  uint64_t *val, uint64_t *block_sums, unsigned long long *d_total, hipStream_t s) {
    dist_hist_kernel<<<grid_of(t.slots), kStThreads, 0, s>>>(t, adjustment, bins);
    dist_flag_bins_kernel<<<grid_of(n_bins), kStThreads, 0, s>>>(bins, n_bins, val);
    scan_exclusive(val, n_bins, block_sums, d_total, s);
    return hipGetLastError();
}

hipError_t launch_store_dist_emit(const uint32_t *bins, uint64_t n_bins, const uint64_t *val, uint64_t adjustment,
                                  uint64_t *d_sizes, uint32_t *d_counts, hipStream_t s) {
    dist_emit_kernel<<<grid_of(n_bins), kStThreads, 0, s>>>(bins, n_bins, val, adjustment, d_sizes, d_counts);
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

hipError_t launch_scrub_flag(const IndexTable &t, const uint8_t *kind, int want_kind, uint64_t *val,
                             uint64_t *block_sums, unsigned long long *d_total, hipStream_t s) {
    scrub_flag_kernel<<<grid_of(t.slots), kStThreads, 0, s>>>(t, kind, want_kind, val);
    scan_exclusive(val, t.slots, block_sums, d_total, s);
    return hipGetLastError();
}

hipError_t launch_scrub_list(const IndexTable &t, const uint8_t *kind, const uint64_t *loc, const uint64_t *val,
                             void *d_chunks, uint8_t *d_digests, uint32_t *d_slot, unsigned long long *d_bytes,
                             hipStream_t s) {
    scrub_list_kernel<<<grid_of(t.slots), kStThreads, 0, s>>>(t, kind, loc, val,
                                                              reinterpret_cast<cdc_chunk_pod *>(d_chunks), d_digests,
                                                              d_slot, d_bytes);
    return hipGetLastError();
}

hipError_t launch_scrub_padsum(const void *d_chunks, uint64_t n, unsigned long long *d_sum, hipStream_t s) {
    if (!n) return hipSuccess;
    scrub_padsum_kernel<<<grid_of(n), kStThreads, 0, s>>>(reinterpret_cast<const cdc_chunk_pod *>(d_chunks), n, d_sum);
    return hipGetLastError();
}

hipError_t launch_scrub_mark(const ScrubState &w, const uint32_t *c_slot, uint64_t nc, const uint64_t *d_first,
                             const void *d_sub, const uint32_t *t_slot, uint64_t n, uint64_t key_base,
                             hipStream_t s) {
    const uint64_t m = nc > n ? nc : n;
    if (!m) return hipSuccess;
    scrub_mark_kernel<<<grid_of(m), kStThreads, 0, s>>>(w, c_slot, nc, d_first,
                                                        reinterpret_cast<const cdc_chunk_pod *>(d_sub), t_slot, n,
                                                        key_base);
    return hipGetLastError();
}

hipError_t launch_store_lookup_x(const IndexTable &t, const ScrubView &v, const uint8_t *d_digests, uint64_t n,
                                 uint32_t *slot_of, uint64_t *cnt, uint64_t *val, unsigned long long *d_res,
                                 hipStream_t s) {
    if (!n) return hipSuccess;
    lookup_x_kernel<<<grid_of(n), kStThreads, 0, s>>>(t, v, d_digests, n, slot_of, cnt, val, d_res);
    return hipGetLastError();
}

hipError_t launch_store_pieces_x(const IndexTable &t, const ScrubView &v, const uint64_t *loc, const uint8_t *arena,
                                 const uint32_t *slot_of, const uint64_t *pstart, const uint64_t *off, uint64_t n,
                                 uint64_t d_out, StorePiece *pieces, uint64_t *tiles, uint64_t n_pieces,
                                 hipStream_t s) {
    if (!n || !n_pieces) return hipSuccess;
    pieces_x_kernel<<<grid_of(n_pieces), kStThreads, 0, s>>>(t, v, loc, (uint64_t)(uintptr_t)arena, slot_of, pstart,
                                                             off, n, d_out, pieces, tiles, n_pieces);
    return hipGetLastError();
}

hipError_t launch_store_spans_x(const IndexTable &t, const uint32_t *slot_of, const uint64_t *off, uint64_t n,
                                void *d_spans, hipStream_t s) {
    if (!n) return hipSuccess;
    spans_x_kernel<<<grid_of(n), kStThreads, 0, s>>>(t, slot_of, off, n, reinterpret_cast<cdc_chunk_pod *>(d_spans));
    return hipGetLastError();
}

hipError_t launch_store_iterate(const IndexTable &t, const ScrubView &v, const uint64_t *val, uint8_t *d_digests,
                                uint8_t *d_kinds, uint64_t *d_lengths, uint64_t *d_key_first, hipStream_t s) {
    iterate_kernel<<<grid_of(t.slots), kStThreads, 0, s>>>(t, v, val, d_digests, d_kinds, d_lengths, d_key_first);
    return hipGetLastError();
}

hipError_t launch_store_key_counts(const IndexTable &t, const ScrubView &v, uint64_t *val, hipStream_t s) {
    key_counts_kernel<<<grid_of(t.slots), kStThreads, 0, s>>>(t, v, val);
    return hipGetLastError();
}

hipError_t launch_store_keys(const IndexTable &t, const ScrubView &v, const uint64_t *val, uint8_t *d_keys,
                             hipStream_t s) {
    keys_kernel<<<grid_of(t.slots), kStThreads, 0, s>>>(t, v, val, d_keys);
    return hipGetLastError();
}

hipError_t launch_retain_refs(const IndexTable &t, const uint8_t *d_digests, uint64_t n, unsigned long long *refs,
                              unsigned long long *d_res, hipStream_t s) {
    if (!n) return hipSuccess;
    retain_refs_kernel<<<grid_of(n), kStThreads, 0, s>>>(t, d_digests, n, refs, d_res);
    return hipGetLastError();
}

hipError_t launch_retain_flag(const IndexTable &t, const unsigned long long *refs, uint64_t *val,
                              uint64_t *block_sums, unsigned long long *d_acc, unsigned long long *d_total,
                              hipStream_t s) {
    retain_flag_kernel<<<grid_of(t.slots), kStThreads, 0, s>>>(t, refs, val, d_acc);
    scan_exclusive(val, t.slots, block_sums, d_total, s);
    return hipGetLastError();
}

hipError_t launch_retain_list(const IndexTable &t, const uint64_t *loc, const unsigned long long *refs,
                              const uint64_t *val, uint64_t *key, uint32_t *slot, hipStream_t s) {
    retain_list_kernel<<<grid_of(t.slots), kStThreads, 0, s>>>(t, loc, refs, val, key, slot);
    return hipGetLastError();
}

hipError_t launch_retain_sort(void *temp, size_t *temp_bytes, const uint64_t *key_in, uint64_t *key_out,
                              const uint32_t *slot_in, uint32_t *slot_out, uint64_t m, unsigned end_bit,
                              hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, *temp_bytes, key_in, key_out, slot_in, slot_out, (size_t)m, 0u, end_bit, s);
}

hipError_t launch_retain_layout(const IndexTable &t, const uint32_t *slot, uint64_t m, uint64_t *newloc,
                                uint64_t *block_sums, uint8_t *d_digests, void *d_chunks, hipStream_t s) {
    if (!m) return hipSuccess;
    retain_gather_kernel<<<grid_of(m), kStThreads, 0, s>>>(t, slot, m, newloc, d_digests,
                                                           reinterpret_cast<cdc_chunk_pod *>(d_chunks));
    scan_exclusive(newloc, m, block_sums, reinterpret_cast<unsigned long long *>(newloc + m), s);
    return hipGetLastError();
}

hipError_t launch_retain_plan(const uint64_t *key, const uint64_t *newloc, uint64_t m, uint64_t w_req,
                              uint64_t max_pad, RetainGroup *groups, uint64_t cap, unsigned long long *d_out,
                              hipStream_t s) {
    retain_plan_kernel<<<1, 64, 0, s>>>(key, newloc, m, w_req, max_pad, groups, cap, d_out);
    return hipGetLastError();
}

hipError_t launch_retain_pieces(const uint64_t *key, const uint64_t *newloc, uint64_t m, const RetainGroup *groups,
                                uint64_t ng, const uint8_t *arena, const uint8_t *bounce, StorePiece *pieces,
                                uint64_t *tstart, uint64_t *block_sums, uint64_t *trel, uint64_t *gtiles,
                                hipStream_t s) {
    if (!m || !ng) return hipSuccess;
    retain_pieces_kernel<<<grid_of(m), kStThreads, 0, s>>>(key, newloc, m, groups, ng, (uint64_t)(uintptr_t)arena,
                                                           (uint64_t)(uintptr_t)bounce, pieces, tstart);
    scan_exclusive(tstart, m, block_sums, reinterpret_cast<unsigned long long *>(tstart + m), s);
    retain_rel_kernel<<<grid_of(m + ng), kStThreads, 0, s>>>(tstart, m, groups, ng, trel, gtiles);
    return hipGetLastError();
}

hipError_t launch_retain_scatter(const uint32_t *old_slot, const uint32_t *new_slot, const uint64_t *newloc,
                                 uint64_t m, uint64_t *new_loc, uint32_t *map, hipStream_t s) {
    if (!m) return hipSuccess;
    retain_scatter_kernel<<<grid_of(m), kStThreads, 0, s>>>(old_slot, new_slot, newloc, m, new_loc, map);
    return hipGetLastError();
}

}  // namespace cdc
