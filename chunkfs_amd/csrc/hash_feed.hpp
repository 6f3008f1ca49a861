// hash_feed.hpp -- what the per-chunk hash kernels (sha256.hip, blake2sp.hip)
// share: how a wave is fed chunks, how a 64-byte block is read, and how the
// resident grid is sized.  What differs stays in the kernels: the byte order of
// the message words (each has its own v_perm selector), the padding and the
// compression.
//
// Work distribution: a lane (SHA-256) or a group of 8 lanes (BLAKE2sp) hashes
// one chunk at a time and keeps the NEXT chunk claimed and described ahead of
// time, in a three-stage pipeline that advances one stage per block step --
// (1) claim an index (one atomic per wave for all that need one), (2) find its
// stream (binary search of the batch's first[] in LDS) and issue the loads of
// its record and its successor's, (3) take it over when the current chunk
// ends.  Each stage's latency (L2 atomic, record loads) then hides behind a
// step of compression instead of stalling the wave at every refill (SHA-256:
// ~2 of 3 steps see a lane finish: 64 lanes, ~65 blocks per 4 KiB chunk).  A
// kernel's loop therefore runs take-over, ChunkFeed::advance (describe, then
// claim), then its block step, in that order.  Waves leave when nothing is
// pending or being hashed anywhere in them and the counter is exhausted.
//
// A block of the message is 17 dwords from the 4-byte-aligned address below
// it, realigned by one v_perm per word; the 68-byte window is read with four
// 16-byte loads and one dword load whenever it cannot run past readable
// memory: inside the chunk, or past its end into the next chunk of the same
// stream when that one is contiguous and >= 68 bytes ("over": every chunk but
// the last one or two of a stream).  Otherwise (a stream's last chunk tail)
// each dword is loaded only if it holds a chunk byte.
#pragma once
#include "sha256.hpp"

namespace cdc {

constexpr uint32_t kHashLdsStreams = 2048;  // stream tables up to this many streams are staged in LDS

// Resident waves only (the counter spreads the chunks over them): one block
// per SIMD-wave slot the kernel's registers allow, and no more blocks than
// the chunks fill at chunks_per_wave each.
template <typename Kernel>
inline hipError_t hash_grid(Kernel kernel, int threads, size_t dyn, uint64_t n_chunks, uint32_t chunks_per_wave,
                            int num_cus, unsigned *grid) {
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, dyn);
    if (e != hipSuccess) return e;
    const uint64_t waves = (n_chunks + chunks_per_wave - 1) / chunks_per_wave;
    const uint64_t per_block = (uint64_t)threads / 64;
    const uint64_t want = (waves + per_block - 1) / per_block;
    const uint64_t cap = (uint64_t)num_cus * (uint64_t)(per_cu > 0 ? per_cu : 1);
    *grid = (unsigned)(want < cap ? want : cap);
    return hipSuccess;
}

typedef const __attribute__((address_space(1))) uint32_t g_u32;
typedef const __attribute__((address_space(1))) uint64_t g_u64c;
// 16-byte loads at a 4-byte-aligned address (a chunk starts at any byte).
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef const __attribute__((address_space(1))) u32x4_a4 g_u32x4_a4;

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_rotateright32(x, n); }
// Three-input XOR in one v_bitop3_b32 (truth table 0x96); LLVM emits two
// v_xor_b32 for the plain expression.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// (kLds) the batch's stream table into tab, the block's (2n+1) * 8 bytes of
// dynamic LDS: first[n+1] ++ base[n], which first / sbase then point to.
template <bool kLds, int kThreads>
__device__ __forceinline__ void stage_stream_table(const ShaBatch &j, uint64_t *tab, const uint64_t *&first,
                                                   const uint64_t *&sbase) {
    first = j.first;
    sbase = j.base;
    if constexpr (kLds) {
        for (uint32_t i = threadIdx.x; i <= 2 * j.n_streams; i += kThreads)
            tab[i] = i <= j.n_streams ? *(g_u64c *)(j.first + i) : *(g_u64c *)(j.base + (i - j.n_streams - 1));
        __syncthreads();
        first = tab;
        sbase = tab + j.n_streams + 1;
    }
}

// The 17 aligned dwords that hold the 64 bytes at offset p of the chunk at src
// (len bytes); returns the byte shift (src + p) & 3 of the block within them.
// p >= len (a padding-only block, an idle lane: len 0) loads nothing and gives
// zeros.  Dwords wholly past the chunk's end are zero in the guarded form and
// whatever follows the chunk in the other: the caller masks its tail.
__device__ __forceinline__ uint32_t load_window(uint32_t (&d)[17], uint64_t src, uint64_t len, uint64_t p, bool over) {
    const uint64_t a = src + p;
    const uint32_t sh = (uint32_t)(a & 3);
    const uint64_t al = a - sh;
    if (p >= len) {
#pragma unroll
        for (int i = 0; i < 17; ++i) d[i] = 0;
    } else if (over || p + 68 <= len) {
        g_u32x4_a4 *q = (g_u32x4_a4 *)al;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32x4_a4 v = q[i];
            d[4 * i] = v.x;
            d[4 * i + 1] = v.y;
            d[4 * i + 2] = v.z;
            d[4 * i + 3] = v.w;
        }
        d[16] = sh ? *(g_u32 *)(al + 64) : 0u;
    } else {
        const uint64_t end = src + len;
#pragma unroll
        for (int i = 0; i < 17; ++i) d[i] = al + 4 * i < end ? *(g_u32 *)(al + 4 * i) : 0u;
    }
    return sh;
}

// The next chunk of a lane (kLanes 1) or of a group of kLanes adjacent lanes
// that hash one chunk together (8: the same state in each of them).
template <uint32_t kLanes>
struct ChunkFeed {
    // lane 0 of every group: the lanes that count in a claim
    static constexpr uint64_t kLeaders = kLanes == 1 ? ~0ull : 0x0101010101010101ull;
    static_assert(kLanes == 1 || kLanes == 8, "one lane or one byte of the ballot per chunk");

    uint32_t nst = 0;  // stage 0 = none, 1 = index claimed, 2 = described, 3 = counter exhausted
    uint64_t ni = 0, nsrc = 0;
    cdc_chunk_pod nc{}, nn{};  // its record, and its successor's in the stream (nhas)
    bool nhas = false;

    __device__ __forceinline__ bool ready() const { return nst == 2; }
    __device__ __forceinline__ bool pending() const { return nst == 1 || nst == 2; }
    // Of a ready() chunk: its index in the batch, its first byte, its length,
    // and whether a 68-byte window may run past its end.
    __device__ __forceinline__ uint64_t index() const { return ni; }
    __device__ __forceinline__ uint64_t src() const { return nsrc + nc.offset; }
    __device__ __forceinline__ uint64_t length() const { return nc.length; }
    __device__ __forceinline__ bool over() const {
        return nhas && nn.offset == nc.offset + nc.length && nn.length >= 68;
    }
    // (3) the caller took the ready() chunk over
    __device__ __forceinline__ void taken() { nst = 0; }

    // Stages 2 and 1, wave-synchronous.
    __device__ __forceinline__ void advance(const ShaBatch &j, const uint64_t *first, const uint64_t *sbase,
                                            uint32_t lane) {
        // (2) describe a claimed index: its stream, and the loads of its record
        if (nst == 1) {
            ni = j.order[ni];  // claims go longest chunk first
            uint32_t lo = 0, hi = j.n_streams;  // largest s with first[s] <= ni
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (first[mid] <= ni) lo = mid; else hi = mid;
            }
            nsrc = sbase[lo];
            nhas = ni + 1 < first[lo + 1];
            nc = j.chunks[ni];
            nn = j.chunks[nhas ? ni + 1 : ni];
            nst = 2;
        }
        // (1) claim indices for the lanes / groups with an empty next stage
        const uint64_t want = __ballot(nst == 0) & kLeaders;
        if (want) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(j.counter, (unsigned long long)__popcll(want));
            base = __shfl(base, 0);
            if (nst == 0) {
                const uint64_t leaders_lt = kLeaders & ((1ull << (lane & ~(kLanes - 1))) - 1);
                ni = base + (uint64_t)__popcll(want & leaders_lt);
                nst = ni < j.n_chunks ? 1u : 3u;
            }
        }
    }
};

}  // namespace cdc
