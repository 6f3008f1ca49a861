// sha256.hip -- SHA-256 (FIPS 180-4) of every chunk of a stream, on gfx950.
//
// The reference fingerprints each chunk with `Sha256Hasher::hash`
// (src/hashers.rs:20-36, sha2 crate), called per chunk in StorageWriter::write
// (src/system/storage.rs:324-329) -- the next-largest cost of its write path
// after chunking.
//
// Layout: one LANE per chunk (a chunk's 64-byte blocks are inherently
// sequential); a launch takes the chunks of many streams at once (a batch:
// cdc_sha256_batch_device), so a 4 GiB archive is one launch of ~1M lanes.
// Chunk lengths vary (min..max), so lanes are refilled dynamically: after
// every block, lanes whose chunk is done take the next chunk indices from a
// global counter, and a wave leaves only when the counter is exhausted and all
// its lanes are idle.  That pipeline, the block loads and the grid size are
// shared with blake2sp.hip (hash_feed.hpp); the claim order (below) is too.
// Each block's 16 big-endian words are built from 17 aligned dwords with one
// v_perm_b32 per word (funnel shift + byte swap in one instruction); the last
// one or two blocks (0x80 terminator, bit length) are masked in registers.
// Integer work only: Ch/Maj and the sigmas' three-way XORs lower to
// v_bitop3_b32, rotations to v_alignbit.
#include "sha256.hpp"

#include <algorithm>

#include "hash_feed.hpp"

namespace cdc {
namespace {

__constant__ uint32_t kK[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

constexpr uint32_t kH0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                             0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};

constexpr int kShaThreads = 256;

// One message block into the state.
__device__ __forceinline__ void compress(uint32_t (&H)[8], uint32_t (&W)[16]) {
    uint32_t a = H[0], b = H[1], c = H[2], d = H[3], e = H[4], f = H[5], g = H[6], h = H[7];
#pragma unroll
    for (int t = 0; t < 64; ++t) {
        uint32_t w;
        if (t < 16) {
            w = W[t];
        } else {
            const uint32_t w15 = W[(t + 1) & 15], w2 = W[(t + 14) & 15];
            const uint32_t s0 = xor3(rotr(w15, 7), rotr(w15, 18), w15 >> 3);
            const uint32_t s1 = xor3(rotr(w2, 17), rotr(w2, 19), w2 >> 10);
            w = W[t & 15] + s0 + W[(t + 9) & 15] + s1;
            W[t & 15] = w;
        }
        const uint32_t S1 = xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25));
        const uint32_t ch = (e & f) ^ (~e & g);
        const uint32_t t1 = h + S1 + ch + kK[t] + w;
        const uint32_t S0 = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22));
        const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
        const uint32_t t2 = S0 + mj;
        h = g;
        g = f;
        f = e;
        e = d + t1;
        d = c;
        c = b;
        b = a;
        a = t1 + t2;
    }
    H[0] += a; H[1] += b; H[2] += c; H[3] += d;
    H[4] += e; H[5] += f; H[6] += g; H[7] += h;
}

__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

// The 16 big-endian message words of block `blk` of the chunk at src (len
// bytes, nblk blocks with the padding), from load_window's 17 dwords by one
// v_perm_b32 per word.  The words of the last one or two blocks (0x80
// terminator, zeros, 64-bit bit length) are masked in registers, without byte
// loops.  Wave-synchronous (the padding mask runs when any lane needs it).
__device__ __forceinline__ void block_words(uint32_t (&W)[16], uint64_t src, uint64_t len, uint64_t blk,
                                            uint64_t nblk, bool over) {
    const uint64_t p = 64 * blk;  // block start within the chunk
    uint32_t d[17];
    const uint32_t sh = load_window(d, src, len, p, over);
    const uint32_t sel = (sh << 24) | ((sh + 1) << 16) | ((sh + 2) << 8) | (sh + 3);
#pragma unroll
    for (int i = 0; i < 16; ++i) W[i] = __builtin_amdgcn_perm(d[i + 1], d[i], sel);
    if (__ballot(p + 64 > len)) {
        // Word i holds message bytes p+4i .. p+4i+3: r = len - (p+4i) of them
        // are data; the first one past the data is 0x80.
        const int64_t r0 = (int64_t)len - (int64_t)p;
        const bool last = blk + 1 == nblk;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t r = r0 - 4 * i;
            const uint32_t rk = (uint32_t)(r < 0 ? 0 : r > 4 ? 4 : r);  // data bytes kept
            const uint32_t rp = (uint32_t)(r < 0 ? 5 : r > 5 ? 5 : r);  // 0x80 position (>= 4: none)
            const uint32_t keep = (uint32_t)~(0xFFFFFFFFull >> (8 * rk));
            const uint32_t pad = (uint32_t)(0x80000000ull >> (8 * rp));
            W[i] = (W[i] & keep) | pad;
        }
        if (last) {
            W[14] = (uint32_t)(len >> 29);  // bit length, big-endian 64-bit
            W[15] = (uint32_t)(len << 3);
        }
    }
}

// One chunk per lane at a time, fed by ChunkFeed<1> (hash_feed.hpp).  (2 chunks
// per lane, their compression chains interleaved: 7.4 vs 6.9 ms per 4 GiB.)
template <bool kLds>
__global__ __launch_bounds__(kShaThreads) void sha256_kernel(const ShaBatch j) {
    extern __shared__ uint64_t tab[];  // (kLds) the stream table
    const uint64_t *first, *sbase;
    stage_stream_table<kLds, kShaThreads>(j, tab, first, sbase);
    const uint32_t lane = threadIdx.x & 63;
    // the lane's chunk (ci ~0: idle, len 0)
    uint64_t ci = ~0ull, src = 0, len = 0, blk = 0, nblk = 0;
    bool over = false;
    uint32_t H[8];
    ChunkFeed<1> next;
    for (;;) {
        // (3) an idle lane takes the next chunk over
        if (next.ready() && ci == ~0ull) {
            ci = next.index();
            src = next.src();
            len = next.length();
            over = next.over();
            blk = 0;
            nblk = (len + 9 + 63) / 64;  // message + 0x80 + 64-bit length, padded
#pragma unroll
            for (int i = 0; i < 8; ++i) H[i] = kH0[i];
            next.taken();
        }
        next.advance(j, first, sbase, lane);
        if (__ballot(next.pending() || ci != ~0ull) == 0) break;  // nothing left anywhere in the wave
        // one block (an idle lane hashes a dummy block: the lanes run in
        // lockstep anyway, and its state is reset at take-over)
        uint32_t W[16];
        block_words(W, src, len, blk, nblk, over);
        compress(H, W);
        if (ci != ~0ull && ++blk == nblk) {
            uint32_t *o = j.digests + 8 * ci;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = bswap(H[i]);  // big-endian digest bytes
            ci = ~0ull;
            len = blk = nblk = 0;
        }
    }
}

// Longest-first claim order (a counting sort of the chunks by length class,
// descending): lanes take chunks from a global counter, and a wave runs until
// its slowest lane is done, so the last chunks a lane takes should be the
// short ones -- in index order a lane's final chunk was as likely 8 KiB as
// 2 KiB, and waves idled up to a whole chunk in their tails.
__device__ __forceinline__ uint32_t len_class(uint64_t len) {
    const uint32_t lz = (uint32_t)__builtin_clzll(len | 1);  // log-linear classes: 8 per octave
    const uint32_t oct = 63 - lz;
    const uint32_t sub = oct >= 3 ? (uint32_t)(len >> (oct - 3)) & 7u : (uint32_t)len & 7u;
    const uint32_t c = oct * 8 + sub;
    return c < kShaBuckets ? kShaBuckets - 1 - c : 0u;  // descending length
}

__global__ __launch_bounds__(256) void sha_hist_kernel(const cdc_chunk_pod *__restrict__ chunks, uint64_t n,
                                                      unsigned long long *hist) {
    __shared__ uint32_t h[kShaBuckets];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        atomicAdd(&h[len_class(chunks[i].length)], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// One block: exclusive scan of the histogram in place (then the scatter's cursors).
__global__ __launch_bounds__(256) void sha_scan_kernel(unsigned long long *hist) {
    __shared__ unsigned long long v[kShaBuckets];
    v[threadIdx.x] = hist[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long acc = 0;
        for (uint32_t k = 0; k < kShaBuckets; ++k) {
            const unsigned long long c = v[k];
            v[k] = acc;
            acc += c;
        }
    }
    __syncthreads();
    hist[threadIdx.x] = v[threadIdx.x];
}

// Block-local scatter: a block takes kShaTile consecutive chunks, counts
// them per class in LDS, reserves each class's run with ONE global atomic
// (822k chunks into ~17 classes with one atomic per chunk took 2.4 ms of
// contention), then places them with LDS atomics.
constexpr uint32_t kShaTile = 4096;

__global__ __launch_bounds__(256) void sha_scatter_kernel(const cdc_chunk_pod *__restrict__ chunks, uint64_t n,
                                                         unsigned long long *cursor, uint32_t *order) {
    __shared__ uint32_t cnt[kShaBuckets];
    __shared__ unsigned long long base[kShaBuckets];
    for (uint64_t t0 = (uint64_t)blockIdx.x * kShaTile; t0 < n; t0 += (uint64_t)gridDim.x * kShaTile) {
        const uint64_t t1 = t0 + kShaTile < n ? t0 + kShaTile : n;
        cnt[threadIdx.x] = 0;
        __syncthreads();
        for (uint64_t i = t0 + threadIdx.x; i < t1; i += 256) atomicAdd(&cnt[len_class(chunks[i].length)], 1u);
        __syncthreads();
        const uint32_t c = cnt[threadIdx.x];
        base[threadIdx.x] = c ? atomicAdd(&cursor[threadIdx.x], (unsigned long long)c) : 0ull;
        cnt[threadIdx.x] = 0;
        __syncthreads();
        for (uint64_t i = t0 + threadIdx.x; i < t1; i += 256) {
            const uint32_t k = len_class(chunks[i].length);
            order[base[k] + atomicAdd(&cnt[k], 1u)] = (uint32_t)i;
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_sha_order(const ShaBatch &b, int num_cus, hipStream_t s) {
    hipError_t e = hipMemsetAsync(b.counter, 0, (1 + kShaBuckets) * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    unsigned long long *hist = b.counter + 1;
    const unsigned sgrid = (unsigned)std::min<uint64_t>((b.n_chunks + 255) / 256, (uint64_t)num_cus * 4);
    sha_hist_kernel<<<sgrid, 256, 0, s>>>(b.chunks, b.n_chunks, hist);
    sha_scan_kernel<<<1, 256, 0, s>>>(hist);
    const unsigned tgrid = (unsigned)std::min<uint64_t>((b.n_chunks + kShaTile - 1) / kShaTile, (uint64_t)num_cus * 4);
    sha_scatter_kernel<<<tgrid, 256, 0, s>>>(b.chunks, b.n_chunks, hist, b.order);
    return hipSuccess;
}

hipError_t launch_sha256(const ShaBatch &b, int num_cus, hipStream_t s) {
    if (!b.n_chunks) return hipSuccess;
    hipError_t e = launch_sha_order(b, num_cus, s);
    if (e != hipSuccess) return e;
    const bool lds = b.n_streams <= kHashLdsStreams;
    const size_t dyn = lds ? (2 * b.n_streams + 1) * sizeof(uint64_t) : 0;
    const auto kernel = lds ? sha256_kernel<true> : sha256_kernel<false>;
    unsigned grid = 0;
    e = hash_grid(kernel, kShaThreads, dyn, b.n_chunks, 64, num_cus, &grid);  // a wave takes 64 chunks at a time
    if (e != hipSuccess) return e;
    kernel<<<grid, kShaThreads, dyn, s>>>(b);
    return hipGetLastError();
}

}  // namespace cdc
