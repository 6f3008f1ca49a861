// pack.hip -- one file of the device file layer as a pack (include/chunkfs_amd.h,
// "Packs"; DESIGN.md "Packs: send and receive"): header, the file's digests and
// lengths, the map span -> carried chunk and back, the chunk offsets, and the
// carried chunks back to back -- the file's distinct slots that the receiver is
// not known to hold, in order of first occurrence.
//
// Packing is the distribution's first-occurrence pass with one more bit per
// slot (excluded), two scans (rank and padded offset of the carried chunks), one
// kernel that writes everything but the data, and the store's copy over a piece
// list for the data.  Unpacking treats the pack as untrusted: the host checks
// the header and the section sizes, one kernel checks every index of the index
// sections before another kernel follows one (the predicates are pack_plan.hpp's,
// each bounding what it reads), and only then are chunks gathered, hashed, put
// and the span table built by the append the file layer already has.
#include "pack.hpp"

namespace cdc {
namespace {

constexpr int kPkThreads = 256;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kPkThreads - 1) / kPkThreads); }

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) v += __shfl_xor(v, k);
    return v;
}

// ---- (a) mark --------------------------------------------------------------------
__global__ __launch_bounds__(kPkThreads) void pack_init_kernel(const uint32_t *__restrict__ slot, uint64_t n,
                                                               uint32_t *excl, uint64_t *firstpos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot[i];
    if (s == kNoSlot) return;
    excl[s] = 0;  // every writer of a slot writes the same values
    firstpos[s] = ~0ull;
}

// Threads [0, n): the file's spans.  Threads [n, n + ns): the spans of `since`,
// whose slots may lie outside the file's: those entries of excl are scratch no
// later step reads.
__global__ __launch_bounds__(kPkThreads) void pack_mark_kernel(const uint32_t *__restrict__ slot, uint64_t n,
                                                               const uint32_t *__restrict__ since_slot, uint64_t ns,
                                                               const uint8_t *__restrict__ have, uint64_t slots,
                                                               uint32_t *excl, uint64_t *firstpos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + ns) return;
    if (i >= n) {
        const uint32_t s = since_slot[i - n];
        if (s < slots) excl[s] = 1;
        return;
    }
    const uint32_t s = slot[i];
    if (s == kNoSlot) return;
    atomicMin((unsigned long long *)&firstpos[s], (unsigned long long)i);
    if (have && have[i]) excl[s] = 1;
}

// ---- (b) carried chunks ----------------------------------------------------------
__global__ __launch_bounds__(kPkThreads) void pack_flag_kernel(const uint32_t *__restrict__ slot,
                                                               const uint64_t *__restrict__ off, uint64_t n,
                                                               const uint32_t *__restrict__ excl,
                                                               const uint64_t *__restrict__ firstpos, uint64_t *rank,
                                                               uint64_t *poff, unsigned long long *acc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t external = 0, bytes = 0;
    if (i < n) {
        const uint32_t s = slot[i];
        const bool out = s == kNoSlot || excl[s] != 0;
        const bool first = !out && firstpos[s] == i;
        const uint64_t len = off[i + 1] - off[i];
        rank[i] = first ? 1 : 0;
        poff[i] = first ? (len + (kPackAlign - 1)) & ~(kPackAlign - 1) : 0;
        external = out ? 1 : 0;
        bytes = first ? len : 0;
    }
    external = wave_sum(external);
    bytes = wave_sum(bytes);
    if ((threadIdx.x & 63) == 0) {
        if (external) atomicAdd(&acc[0], (unsigned long long)external);
        if (bytes) atomicAdd(&acc[1], (unsigned long long)bytes);
    }
}

// ---- (c) header and sections -----------------------------------------------------
// rank / poff are scanned.  Thread 0 also writes the header, the entry that
// closes chunk_off and the padding of the 8-byte sections; the thread of a
// carried chunk's first span writes its chunk_span / chunk_off entries, the
// zero bytes after its data, and its piece.
__global__ __launch_bounds__(kPkThreads) void pack_write_kernel(SpanTable t, uint64_t n,
                                                                const uint32_t *__restrict__ excl,
                                                                const uint64_t *__restrict__ firstpos,
                                                                const uint64_t *__restrict__ rank,
                                                                const uint64_t *__restrict__ poff, PackHeader h,
                                                                PackLayout l, uint8_t *pack, uint64_t arena,
                                                                StorePiece *pieces, uint64_t *tiles) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t *span_length = reinterpret_cast<uint64_t *>(pack + l.length);
    uint64_t *span_chunk = reinterpret_cast<uint64_t *>(pack + l.span_chunk);
    uint64_t *chunk_span = reinterpret_cast<uint64_t *>(pack + l.chunk_span);
    uint64_t *chunk_off = reinterpret_cast<uint64_t *>(pack + l.chunk_off);
    if (i == 0) {
        uint64_t *w = reinterpret_cast<uint64_t *>(pack);
        w[0] = h.magic;
        w[1] = (uint64_t)h.version | ((uint64_t)h.flags << 32);
        w[2] = h.file_size;
        w[3] = h.n_spans;
        w[4] = h.n_chunks;
        w[5] = h.external_spans;
        w[6] = h.data_bytes;
        w[7] = h.total_bytes;
        if (h.n_spans) {  // a pack without spans is its header
            chunk_off[h.n_chunks] = h.data_bytes;
            if (h.n_spans & 1) span_length[h.n_spans] = 0, span_chunk[h.n_spans] = 0;
            if (h.n_chunks & 1) chunk_span[h.n_chunks] = 0;
            else chunk_off[h.n_chunks + 1] = 0;
        }
    }
    if (i >= n) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(t.digest + 32 * i);
    uint4 *dst = reinterpret_cast<uint4 *>(pack + l.digest + 32 * i);
    dst[0] = src[0];
    dst[1] = src[1];
    const uint64_t len = t.off[i + 1] - t.off[i];
    span_length[i] = len;
    const uint32_t s = t.slot[i];
    if (s == kNoSlot || excl[s] != 0) {
        span_chunk[i] = kPackExternal;
        return;
    }
    const uint64_t fp = firstpos[s], k = rank[fp];
    span_chunk[i] = k;
    if (fp != i) return;
    const uint64_t at = poff[i];
    chunk_span[k] = i;
    chunk_off[k] = at;
    uint8_t *data = pack + l.data + at;
    const uint64_t padded = (len + (kPackAlign - 1)) & ~(kPackAlign - 1);
    for (uint64_t b = len; b < padded; ++b) data[b] = 0;
    pieces[k] = StorePiece{arena + t.loc[i], (uint64_t)(uintptr_t)data, len};
    tiles[k] = (len + (kStoreTile - 1)) / kStoreTile;  // data is 16-byte aligned
}

// ---- unpack: validation ------------------------------------------------------------
__device__ __forceinline__ void pack_fail(PackResult *r, uint32_t check, uint64_t index) {
    atomicAdd(&r->count[check], 1ull);
    atomicMin(&r->first[check], (unsigned long long)index);
}

__global__ __launch_bounds__(kPkThreads) void pack_validate_kernel(PackView v, uint64_t threads, PackResult *r) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    PackSum sum{0, 0};
    uint64_t externals = 0;
    if (i < threads) {
        if (i < v.n_chunks) {
            if (!pack_ok_chunk_span(v, i)) pack_fail(r, kPackChunkSpanCheck, i);
            if (!pack_ok_backref(v, i)) pack_fail(r, kPackBackrefCheck, i);
            if (!pack_ok_chunk_off(v, i)) pack_fail(r, kPackChunkOffCheck, i);
        }
        if (i < v.n_spans) {
            if (!pack_ok_span_chunk(v, i)) pack_fail(r, kPackSpanChunkCheck, i);
            if (!pack_ok_same(v, i)) pack_fail(r, kPackSameCheck, i);
            sum.low = v.length[i];
            externals = v.span_chunk[i] == kPackExternal ? 1 : 0;
        }
        if (i == 0 && !pack_ok_data_bytes(v)) pack_fail(r, kPackDataBytesCheck, v.n_chunks);
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        PackSum o;
        o.low = __shfl_xor(sum.low, k);
        o.wraps = __shfl_xor(sum.wraps, k);
        sum = pack_sum_add(sum, o);
    }
    externals = wave_sum(externals);
    if ((threadIdx.x & 63) == 0) {
        if (sum.low) {
            const unsigned long long old = atomicAdd(&r->sum_low, (unsigned long long)sum.low);
            if (old + sum.low < old) sum.wraps += 1;
        }
        if (sum.wraps) atomicAdd(&r->sum_wraps, (unsigned long long)sum.wraps);
        if (externals) atomicAdd(&r->externals, (unsigned long long)externals);
    }
}

// ---- unpack: lookup ------------------------------------------------------------------
__device__ __forceinline__ bool same_digest(const uint8_t *a, const uint8_t *b) {
    const uint4 *x = reinterpret_cast<const uint4 *>(a), *y = reinterpret_cast<const uint4 *>(b);
    const uint4 x0 = x[0], x1 = x[1], y0 = y[0], y1 = y[1];
    return x0.x == y0.x && x0.y == y0.y && x0.z == y0.z && x0.w == y0.w &&
           x1.x == y1.x && x1.y == y1.y && x1.z == y1.z && x1.w == y1.w;
}

// The store's lookup (store.hip lookup_kernel) with the slot as its answer.
__global__ __launch_bounds__(kPkThreads) void pack_lookup_kernel(IndexTable t, PackView v, uint32_t *slot,
                                                                 PackResult *r) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n_spans) return;
    const uint8_t *d = v.digest + 32 * i;
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
    slot[i] = hit;
    if (v.span_chunk[i] != kPackExternal) return;
    if (hit == kNoSlot) {
        atomicAdd(&r->missing, 1ull);
        atomicMin(&r->missing_first, (unsigned long long)i);
    } else if (t.length[hit] != v.length[i]) {
        atomicAdd(&r->mislen, 1ull);
        atomicMin(&r->mislen_first, (unsigned long long)i);
    }
}

// ---- unpack: the carried chunks --------------------------------------------------------
__global__ __launch_bounds__(kPkThreads) void pack_gather_kernel(PackView v, cdc_chunk_pod *chunks,
                                                                 uint8_t *digests) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= v.n_chunks) return;
    const uint64_t i = v.chunk_span[k];  // < n_spans: validated
    chunks[k] = cdc_chunk_pod{v.chunk_off[k], v.length[i]};
    const uint4 *src = reinterpret_cast<const uint4 *>(v.digest + 32 * i);
    uint4 *dst = reinterpret_cast<uint4 *>(digests + 32 * k);
    dst[0] = src[0];
    dst[1] = src[1];
}

__global__ __launch_bounds__(kPkThreads) void pack_verify_kernel(const uint8_t *__restrict__ sha,
                                                                 const uint8_t *__restrict__ digests, uint64_t n,
                                                                 PackResult *r) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (same_digest(sha + 32 * k, digests + 32 * k)) return;
    atomicAdd(&r->mismatch, 1ull);
    atomicMin(&r->mismatch_first, (unsigned long long)k);
}

__global__ __launch_bounds__(kPkThreads) void pack_slots_kernel(PackView v, const uint32_t *__restrict__ slot_of,
                                                                uint32_t *slot) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n_spans) return;
    const uint64_t c = v.span_chunk[i];  // ~0 or < n_chunks: validated
    if (c != kPackExternal) slot[i] = slot_of[c];
}

}  // namespace

hipError_t launch_pack_mark(const SpanTable &t, uint64_t n, const uint32_t *since_slot, uint64_t ns,
                            const uint8_t *have, uint64_t slots, uint32_t *excl, uint64_t *firstpos, uint64_t *rank,
                            uint64_t *poff, uint64_t *bs_rank, uint64_t *bs_off, unsigned long long *d_acc,
                            unsigned long long *h_out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_acc, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    pack_init_kernel<<<grid_of(n), kPkThreads, 0, s>>>(t.slot, n, excl, firstpos);
    pack_mark_kernel<<<grid_of(n + ns), kPkThreads, 0, s>>>(t.slot, n, since_slot, ns, have, slots, excl, firstpos);
    pack_flag_kernel<<<grid_of(n), kPkThreads, 0, s>>>(t.slot, t.off, n, excl, firstpos, rank, poff, d_acc);
    e = launch_store_scan(rank, n, bs_rank, h_out, s);
    if (e != hipSuccess) return e;
    return launch_store_scan(poff, n, bs_off, h_out + 1, s);
}

hipError_t launch_pack_write(const SpanTable &t, uint64_t n, const uint32_t *excl, const uint64_t *firstpos,
                             const uint64_t *rank, const uint64_t *poff, const PackHeader &h, const PackLayout &l,
                             uint8_t *d_pack, uint64_t arena, StorePiece *pieces, uint64_t *tstart,
                             uint64_t *block_sums, hipStream_t s) {
    pack_write_kernel<<<grid_of(n ? n : 1), kPkThreads, 0, s>>>(t, n, excl, firstpos, rank, poff, h, l, d_pack, arena,
                                                              pieces, tstart);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !h.n_chunks) return e;
    e = launch_store_scan(tstart, h.n_chunks, block_sums, nullptr, s);
    if (e != hipSuccess) return e;
    return launch_store_copy(pieces, tstart, h.n_chunks, h.data_bytes / kStoreTile + h.n_chunks,
                             block_sums + store_scan_blocks(h.n_chunks), s);
}

hipError_t pack_result_preset(PackResult *d_res, hipStream_t s) {
    static PackResult preset = [] {
        PackResult p{};
        for (uint32_t c = 0; c < kPackChecks; ++c) p.first[c] = ~0ull;
        p.missing_first = p.mislen_first = p.mismatch_first = ~0ull;
        return p;
    }();
    return hipMemcpyAsync(d_res, &preset, sizeof preset, hipMemcpyHostToDevice, s);
}

hipError_t launch_pack_validate(const PackView &v, PackResult *d_res, hipStream_t s) {
    uint64_t threads = v.n_spans > v.n_chunks ? v.n_spans : v.n_chunks;
    if (!threads) threads = 1;
    pack_validate_kernel<<<grid_of(threads), kPkThreads, 0, s>>>(v, threads, d_res);
    return hipGetLastError();
}

hipError_t launch_pack_lookup(const IndexTable &t, const PackView &v, uint32_t *slot, PackResult *d_res,
                              hipStream_t s) {
    if (!v.n_spans) return hipSuccess;
    pack_lookup_kernel<<<grid_of(v.n_spans), kPkThreads, 0, s>>>(t, v, slot, d_res);
    return hipGetLastError();
}

hipError_t launch_pack_gather(const PackView &v, void *d_chunks, uint8_t *d_digests, hipStream_t s) {
    if (!v.n_chunks) return hipSuccess;
    pack_gather_kernel<<<grid_of(v.n_chunks), kPkThreads, 0, s>>>(v, static_cast<cdc_chunk_pod *>(d_chunks),
                                                                 d_digests);
    return hipGetLastError();
}

hipError_t launch_pack_verify(const uint8_t *sha, const uint8_t *digests, uint64_t n_chunks, PackResult *d_res,
                              hipStream_t s) {
    if (!n_chunks) return hipSuccess;
    pack_verify_kernel<<<grid_of(n_chunks), kPkThreads, 0, s>>>(sha, digests, n_chunks, d_res);
    return hipGetLastError();
}

hipError_t launch_pack_slots(const PackView &v, const uint32_t *slot_of, uint32_t *slot, hipStream_t s) {
    if (!v.n_spans) return hipSuccess;
    pack_slots_kernel<<<grid_of(v.n_spans), kPkThreads, 0, s>>>(v, slot_of, slot);
    return hipGetLastError();
}

}  // namespace cdc
