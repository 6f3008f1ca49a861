// blake2sp.hip -- BLAKE2sp (RFC 7693's BLAKE2s in its 8-way tree form) of every
// chunk of a batch, on gfx950: the second chunk hasher (DESIGN.md "Hashers").
//
// BLAKE2sp deals a message's 64-byte blocks round-robin to 8 leaves (block k
// to leaf k mod 8), hashes each leaf with BLAKE2s (10 rounds per block) and
// hashes the 8 leaf digests with a 4-block root.  Where SHA-256 is one serial
// chain per chunk, a chunk here is 8 independent chains an eighth as long.
//
// Layout: 8 adjacent lanes form one chunk GROUP, lane g of the group is leaf
// g, a wave carries 8 chunks.  In step j the group reads blocks 8j .. 8j+7 of
// its chunk (512 contiguous bytes) and every lane compresses its own; after
// the last leaf step the group spends 4 more steps on the root, in which lane
// 0 compresses the leaf digests (read from its neighbours by ds_bpermute) and
// the other 7 lanes idle.  Work distribution is the SHA-256 kernel's at group
// granularity (hash_feed.hpp, ChunkFeed<8>): a resident grid, the
// longest-first claim order (launch_sha_order), and groups that refill from
// the global counter after every step through the claim / describe /
// take-over pipeline.
//
// Message words are little-endian, so a block is 17 aligned dwords funnelled
// by one v_perm per word with no byte swap; the load forms are the shared
// load_window's.
#include "blake2sp.hpp"

#include <algorithm>

#include "hash_feed.hpp"

namespace cdc {
namespace {

constexpr uint32_t kIV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                             0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
constexpr uint8_t kSigma[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

// Parameter words 0 and 3 (RFC 7693 §2.5): digest length 32, no key, fanout 8,
// depth 2; inner length 32 with node depth 0 (a leaf) or 1 (the root).  Word 1
// (leaf length) is 0 and word 2 is the node offset: the leaf number, 0 for the
// root.
constexpr uint32_t kParam0 = 0x02080020u;
constexpr uint32_t kParam3Leaf = 0x20000000u, kParam3Root = 0x20010000u;

constexpr int kB2Threads = 256;
// One BLAKE2s compression of block m into h: byte counter t, finalisation
// flags f0 (last block of the node) and f1 (last node of its layer).
__device__ __forceinline__ void compress(uint32_t (&h)[8], const uint32_t (&m)[16], uint64_t t, uint32_t f0,
                                         uint32_t f1) {
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = h[i];
        v[i + 8] = kIV[i];
    }
    v[12] ^= (uint32_t)t;
    v[13] ^= (uint32_t)(t >> 32);
    v[14] ^= f0;
    v[15] ^= f1;
#define CDC_B2_G(a, b, c, d, x, y)     \
    v[a] = v[a] + v[b] + (x);          \
    v[d] = rotr(v[d] ^ v[a], 16);      \
    v[c] = v[c] + v[d];                \
    v[b] = rotr(v[b] ^ v[c], 12);      \
    v[a] = v[a] + v[b] + (y);          \
    v[d] = rotr(v[d] ^ v[a], 8);       \
    v[c] = v[c] + v[d];                \
    v[b] = rotr(v[b] ^ v[c], 7);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        CDC_B2_G(0, 4, 8, 12, m[kSigma[r][0]], m[kSigma[r][1]])
        CDC_B2_G(1, 5, 9, 13, m[kSigma[r][2]], m[kSigma[r][3]])
        CDC_B2_G(2, 6, 10, 14, m[kSigma[r][4]], m[kSigma[r][5]])
        CDC_B2_G(3, 7, 11, 15, m[kSigma[r][6]], m[kSigma[r][7]])
        CDC_B2_G(0, 5, 10, 15, m[kSigma[r][8]], m[kSigma[r][9]])
        CDC_B2_G(1, 6, 11, 12, m[kSigma[r][10]], m[kSigma[r][11]])
        CDC_B2_G(2, 7, 8, 13, m[kSigma[r][12]], m[kSigma[r][13]])
        CDC_B2_G(3, 4, 9, 14, m[kSigma[r][14]], m[kSigma[r][15]])
    }
#undef CDC_B2_G
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = xor3(h[i], v[i], v[i + 8]);
}

// The 16 little-endian message words of the 64 bytes at offset p of the chunk
// at src (len bytes): zeros from the chunk's end on (a final partial block goes
// to its leaf zero-filled; p >= len gives an all-zero block and loads nothing).
// `over`: the 68-byte window may run past the chunk's end (hash_feed.hpp).
// Wave-synchronous (the tail mask runs when any lane needs it).
__device__ __forceinline__ void block_words_le(uint32_t (&W)[16], uint64_t src, uint64_t len, uint64_t p, bool over) {
    uint32_t d[17];
    const uint32_t sh = load_window(d, src, len, p, over);
    const uint32_t sel = ((sh + 3) << 24) | ((sh + 2) << 16) | ((sh + 1) << 8) | sh;
#pragma unroll
    for (int i = 0; i < 16; ++i) W[i] = __builtin_amdgcn_perm(d[i + 1], d[i], sel);
    if (__ballot(p < len && p + 64 > len)) {
        // Word i holds chunk bytes p+4i .. p+4i+3, the first in its low byte:
        // r = len - (p+4i) of them are data.
        const int64_t r0 = p < len ? (int64_t)(len - p) : 64;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t r = r0 - 4 * i;
            const uint32_t rk = (uint32_t)(r < 0 ? 0 : r > 4 ? 4 : r);  // data bytes kept
            W[i] &= (uint32_t)~(0xFFFFFFFFull << (8 * rk));
        }
    }
}

template <bool kLds>
__global__ __launch_bounds__(kB2Threads) void blake2sp_kernel(const ShaBatch j) {
    extern __shared__ uint64_t tab[];  // (kLds) the stream table
    const uint64_t *first, *sbase;
    stage_stream_table<kLds, kB2Threads>(j, tab, first, sbase);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = lane & 7;        // the lane's leaf
    const uint32_t glead = lane & ~7u;  // lane 0 of its group
    // The group's chunk (the same in its 8 lanes; ci ~0: idle): steps 0 ..
    // nsteps-1 hash the leaves, nsteps .. nsteps+3 the root.
    uint64_t ci = ~0ull, src = 0, len = 0, nb = 0, step = 0, nsteps = 0;
    bool over = false;
    uint32_t h[8], dg[8];  // the running state; the lane's finished leaf digest
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = dg[i] = 0;
    ChunkFeed<8> next;
    for (;;) {
        // (3) an idle group takes the next chunk over
        if (next.ready() && ci == ~0ull) {
            ci = next.index();
            src = next.src();
            len = next.length();
            over = next.over();
            nb = (len + 63) / 64;
            nsteps = nb ? (nb + 7) / 8 : 1;  // (an empty chunk still finalises 8 empty leaves)
            step = 0;
            next.taken();
        }
        next.advance(j, first, sbase, lane);
        const bool have = ci != ~0ull;
        if (__ballot(have || next.pending()) == 0) break;  // nothing left anywhere in the wave
        if (__ballot(have) == 0) continue;  // (the pipeline is still filling)
        // One step of every group: a leaf block per lane, or a root block in
        // lane 0.  Lanes with nothing to do compress a zero block and keep
        // their state: the lanes run in lockstep anyway.
        const bool root = have && step >= nsteps;
        const uint32_t rb = root ? (uint32_t)(step - nsteps) : 0u;  // the root block, 0..3
        const uint64_t k = 8 * step + g;                            // the leaf block
        const bool leaf = have && !root && (k < nb || step == 0);   // (step 0: empty leaves finalise too)
        if (have && step == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = kIV[i];
            h[0] ^= kParam0;
            h[2] ^= g;
            h[3] ^= kParam3Leaf;
        }
        if (root && rb == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = kIV[i];
            h[0] ^= kParam0;
            h[3] ^= kParam3Root;
        }
        uint32_t W[16];
        block_words_le(W, src, leaf ? len : 0, 64 * k, over);
        if (__ballot(root)) {
            // root block rb = the digests of leaves 2rb and 2rb+1
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t w = (uint32_t)__shfl((int)dg[i & 7], (int)(glead + 2 * rb + (i >> 3)));
                if (root) W[i] = w;
            }
        }
        uint64_t t;
        bool fin;
        if (root) {
            t = 64 * (uint64_t)(rb + 1);
            fin = rb == 3;
        } else {
            const uint64_t rest = k < nb ? len - 64 * k : 0;  // bytes of the chunk from this block on
            t = k < nb ? 64 * step + (rest < 64 ? rest : 64) : 0;
            fin = k + 8 >= nb;  // the leaf has no later block
        }
        const bool act = leaf || (root && g == 0);
        uint32_t hn[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) hn[i] = h[i];
        compress(hn, W, t, fin ? ~0u : 0u, fin && (root || g == 7) ? ~0u : 0u);
        if (act) {
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = hn[i];
        }
        if (leaf && fin) {
#pragma unroll
            for (int i = 0; i < 8; ++i) dg[i] = hn[i];
        }
        if (have) {
            if (root && rb == 3) {
                if (g == 0) {
                    uint32_t *o = j.digests + 8 * ci;
#pragma unroll
                    for (int i = 0; i < 8; ++i) o[i] = hn[i];  // little-endian digest bytes
                }
                ci = ~0ull;
                len = nb = nsteps = 0;
            }
            ++step;
        }
    }
}

}  // namespace

hipError_t launch_blake2sp(const ShaBatch &b, int num_cus, hipStream_t s) {
    if (!b.n_chunks) return hipSuccess;
    hipError_t e = launch_sha_order(b, num_cus, s);
    if (e != hipSuccess) return e;
    const bool lds = b.n_streams <= kHashLdsStreams;
    const size_t dyn = lds ? (2 * b.n_streams + 1) * sizeof(uint64_t) : 0;
    const auto kernel = lds ? blake2sp_kernel<true> : blake2sp_kernel<false>;
    unsigned grid = 0;
    e = hash_grid(kernel, kB2Threads, dyn, b.n_chunks, 8, num_cus, &grid);  // a wave takes 8 chunks at a time
    if (e != hipSuccess) return e;
    kernel<<<grid, kB2Threads, dyn, s>>>(b);
    return hipGetLastError();
}

}  // namespace cdc
