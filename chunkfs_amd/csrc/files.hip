// files.hip -- device file layer: per-file span tables over the chunk store.
//
// Mirrors the reference's FileLayer (src/system/file_layer.rs): a file is the
// ordered span list {hash, offset, len} (file_layer.rs:9-23); write appends
// spans (file_layer.rs:136-148), read_complete returns them all
// (file_layer.rs:127-133), read takes whole spans from the handle's cursor
// while their total stays within one segment (file_layer.rs:152-175), and
// chunk_count_distribution counts the spans of each hash over all but the last
// span (file_layer.rs:188-206).  pread -- a byte range -- is this layer's own.
//
// Layout: one span table per file, structure of arrays in HBM: the n + 1 byte
// offsets (off[i + 1] - off[i] is span i's length; every search runs over
// them), the 32-byte digests, and per span the table slot and arena offset the
// store resolved when the span was written.  A put never moves stored bytes,
// and a collect (the one call that does) rewrites both in every table, so a
// read goes from span to bytes with no digest lookup.
//
// Every read form is the same four steps with no host wait between them: one
// thread per request resolves its span range by binary search in the offsets;
// a scan over the span counts gives each request its first piece; one thread
// per piece finds its request by binary search and writes the trimmed {src,
// dst, len} and its tile count; the tile scan and the store's copy kernel
// (store.hip) follow, the tile total read on the device.
//
// Once the store holds target-kind containers (the scrub stage, store.hpp
// ScrubView) the chain has one more level: the spans of a request become span
// records, a target-kind span yields one piece per key, a range trims its two
// end spans by binary search over the per-key offsets, and the exact piece
// count goes to the host before the copy.  The chain above is untouched.
//
// get_to_dedup_ratio (file_layer.rs:208-268) derives a file from another one's
// unique spans: the distribution's first-occurrence flags and scan give the
// unique list as span indices, a scan of its lengths gives the cycle's prefix
// sums, and a gather writes the new table with true offsets.  verify
// (src/bench/mod.rs:241-275) is the read chain with the store's compare kernel
// as its last step.
//
// diff (cdc_files_diff_device; not in the reference, DESIGN.md "Snapshots and
// diffs") compares two files of the layer.  The boundaries of both tables are
// ranked into pieces, each inside one span of either file; a piece whose spans
// name one slot at one offset is one arena address and is skipped; the others
// become a piece list for the store's diff_mask_kernel, one bit per byte; a
// wave per tile turns the mask into run starts and ends, a scan ranks them and
// the emit maps (tile, bit) back to file offsets.  The arithmetic is
// diff_plan.hpp's.
#include "files.hpp"

#include "diff_plan.hpp"
#include "read_plan.hpp"
#include "splice_plan.hpp"

namespace cdc {
namespace {

constexpr int kFlThreads = 256;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kFlThreads - 1) / kFlThreads); }

// ---- append --------------------------------------------------------------------
// stat[0] = min over the spans of length - 1 (a length-0 span wraps to the
// maximum and leaves it alone), stat[1] += length-0 spans: from these the host
// bounds how many spans a byte range can touch.  One atomic per wave each.
__global__ __launch_bounds__(kFlThreads) void span_len_kernel(const uint32_t *__restrict__ slot_of,
                                                              const uint64_t *__restrict__ tbl_length, uint64_t n,
                                                              uint64_t *val, unsigned long long *stat) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t least = ~0ull, zeros = 0;
    if (i < n) {
        const uint32_t s = slot_of[i];
        const uint64_t len = s == kNoSlot ? 0 : tbl_length[s];  // the stored chunk's length: what a read may copy
        val[i] = len;
        least = len - 1;
        zeros = len == 0;
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const uint64_t o = __shfl_xor(least, k);
        least = o < least ? o : least;
        zeros += __shfl_xor(zeros, k);
    }
    if ((threadIdx.x & 63) == 0) {
        if (least != ~0ull) atomicMin(&stat[0], (unsigned long long)least);
        if (zeros) atomicAdd(&stat[1], (unsigned long long)zeros);
    }
}

// val = exclusive scan of the span lengths, *total their sum.  Thread n writes
// the new end offset.
__global__ __launch_bounds__(kFlThreads) void append_kernel(SpanTable t, uint64_t n0, uint64_t size0,
                                                            const uint32_t *__restrict__ slot_of,
                                                            const uint64_t *__restrict__ tbl_loc,
                                                            const uint8_t *__restrict__ digests, uint64_t n,
                                                            const uint64_t *__restrict__ val,
                                                            const uint64_t *__restrict__ total) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        t.off[n0 + n] = size0 + *total;
        return;
    }
    const uint32_t s = slot_of[i];
    t.off[n0 + i] = size0 + val[i];
    t.slot[n0 + i] = s;
    t.loc[n0 + i] = s == kNoSlot ? 0 : tbl_loc[s];
    const uint4 *src = reinterpret_cast<const uint4 *>(digests + 32 * i);
    uint4 *dst = reinterpret_cast<uint4 *>(t.digest + 32 * (n0 + i));
    dst[0] = src[0];
    dst[1] = src[1];
}

// ---- segmented append (cdc_files_write_batch_device) -----------------------------
// The m spans of one put belong to nfiles files: file f owns spans [first[f],
// first[f + 1]).  Files without spans make runs of equal entries in first[]; the
// owner of span i is the last f with first[f] <= i (i < first[nfiles], so that f
// has first[f + 1] > i).
__device__ __forceinline__ uint64_t file_of_span(const uint64_t *__restrict__ first, uint64_t nfiles, uint64_t i) {
    uint64_t a = 0, b = nfiles;
    while (b - a > 1) {
        const uint64_t mid = (a + b) >> 1;
        if (first[mid] <= i) a = mid;
        else b = mid;
    }
    return a;
}

// span_len_kernel with per-file statistics.  A wave's lanes may belong to
// several files: the lanes that share the leader's file reduce together and
// retire with one atomic each (as dist_hist_kernel does on the leader's bin).
__global__ __launch_bounds__(kFlThreads) void batch_len_kernel(const uint32_t *__restrict__ slot_of,
                                                               const uint64_t *__restrict__ tbl_length,
                                                               const uint64_t *__restrict__ first, uint64_t nfiles,
                                                               uint64_t m, uint64_t *val, AppendStat *stat) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool todo = i < m;
    uint64_t least = ~0ull, zeros = 0, f = 0;
    if (todo) {
        const uint32_t s = slot_of[i];
        const uint64_t len = s == kNoSlot ? 0 : tbl_length[s];
        val[i] = len;
        least = len - 1;
        zeros = len == 0;
        f = file_of_span(first, nfiles, i);
    }
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long left = __ballot(todo);
    while (left) {  // wave-uniform: every lane takes part in the shuffles
        const uint32_t leader = (uint32_t)__builtin_ctzll(left);
        const uint64_t lead_file = __shfl(f, (int)leader);
        const bool mine = todo && f == lead_file;
        const unsigned long long same = __ballot(mine);
        uint64_t l = mine ? least : ~0ull, z = mine ? zeros : 0;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const uint64_t o = __shfl_xor(l, k);
            l = o < l ? o : l;
            z += __shfl_xor(z, k);
        }
        if (lane == leader) {
            if (l != ~0ull) atomicMin(&stat[lead_file].least, (unsigned long long)l);
            if (z) atomicAdd(&stat[lead_file].zeros, (unsigned long long)z);
        }
        if (mine) todo = false;
        left &= ~same;
    }
}

// val = exclusive scan of all m lengths, *total their sum.  Threads [0, m): span
// i of file f goes to entry n0_f + (i - first[f]) at offset size0_f + val[i] -
// val[first[f]].  Threads [m, m + nfiles): file f's closing offset and byte
// total; a file without spans is left alone (it may have no table).
__global__ __launch_bounds__(kFlThreads) void batch_append_kernel(const AppendDst *__restrict__ dst,
                                                                  const uint64_t *__restrict__ first,
                                                                  uint64_t nfiles, uint64_t m,
                                                                  const uint32_t *__restrict__ slot_of,
                                                                  const uint64_t *__restrict__ tbl_loc,
                                                                  const uint8_t *__restrict__ digests,
                                                                  const uint64_t *__restrict__ val,
                                                                  const uint64_t *__restrict__ total,
                                                                  AppendStat *stat) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m + nfiles) return;
    if (i >= m) {
        const uint64_t f = i - m, lo = first[f], hi = first[f + 1];
        if (hi == lo) return;
        const AppendDst d = dst[f];
        const uint64_t bytes = (hi < m ? val[hi] : *total) - val[lo];
        d.t.off[d.n0 + (hi - lo)] = d.size0 + bytes;
        stat[f].bytes = bytes;
        return;
    }
    const uint64_t f = file_of_span(first, nfiles, i), lo = first[f];
    const AppendDst d = dst[f];
    const uint64_t j = d.n0 + (i - lo);
    const uint32_t s = slot_of[i];
    d.t.off[j] = d.size0 + (val[i] - val[lo]);
    d.t.slot[j] = s;
    d.t.loc[j] = s == kNoSlot ? 0 : tbl_loc[s];
    const uint4 *src = reinterpret_cast<const uint4 *>(digests + 32 * i);
    uint4 *to = reinterpret_cast<uint4 *>(d.t.digest + 32 * j);
    to[0] = src[0];
    to[1] = src[1];
}

// ---- the range planner ---------------------------------------------------------
// single (nullable; a call of one request): the scan over one count is the
// count itself, so it goes straight to *single and the request's first piece is 0.
__global__ __launch_bounds__(kFlThreads) void resolve_kernel(const ReadReq *__restrict__ req, uint64_t nreq,
                                                             ReadPlan *plan, uint64_t *cnt, uint64_t *single,
                                                             ReadResult *h_res) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreq) return;
    const ReadReq q = req[r];
    const ReadSpans x = read_resolve(q.off, q.n, q.kind, q.a, q.b, q.cap);
    plan[r] = ReadPlan{x.lo, x.hi, x.first};
    if (single) {
        cnt[r] = 0;
        *single = x.count;
    } else {
        cnt[r] = x.count;
    }
    h_res[r] = ReadResult{x.hi - x.lo, x.first, x.count};
}

// pstart = exclusive scan of the span counts, *total_pieces their sum.  Threads
// past the total write empty pieces, so the tile scan runs over max_pieces.
__global__ __launch_bounds__(kFlThreads) void pieces_kernel(const ReadReq *__restrict__ req, uint64_t nreq,
                                                            const ReadPlan *__restrict__ plan,
                                                            const uint64_t *__restrict__ pstart,
                                                            const uint64_t *__restrict__ total_pieces,
                                                            uint64_t arena, StorePiece *pieces, uint64_t *tiles,
                                                            uint64_t max_pieces) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= max_pieces) return;
    StorePiece pc{0, 0, 0};
    uint64_t t = 0;
    if (p < *total_pieces) {
        uint64_t a = 0, b = nreq;  // last request r with pstart[r] <= p (requests of no pieces share a start)
        while (b - a > 1) {
            const uint64_t mid = (a + b) >> 1;
            if (pstart[mid] <= p) a = mid;
            else b = mid;
        }
        const ReadReq q = req[a];
        const ReadPlan pl = plan[a];
        const uint64_t k = p - pstart[a], i = pl.first + k;
        const uint64_t s0 = q.off[i], s1 = q.off[i + 1];
        // Only the first and last piece of a range are trimmed.
        const uint64_t from = s0 > pl.lo ? s0 : pl.lo, to = s1 < pl.hi ? s1 : pl.hi;
        const uint64_t len = to > from ? to - from : 0;
        pc.src = arena + q.loc[i] + (from - s0);
        pc.dst = q.dst + (from - pl.lo);
        pc.len = len;
        t = len ? ((pc.dst & (kStoreAlign - 1)) + len + (kStoreTile - 1)) / kStoreTile : 0;
        if (q.spans) reinterpret_cast<cdc_chunk_pod *>(q.spans)[k] = cdc_chunk_pod{from - pl.lo, len};
    }
    pieces[p] = pc;
    tiles[p] = t;
}

// ---- the scrubbed state: span -> pieces ------------------------------------------
// pstart = exclusive scan of the span counts, *total_spans their sum.  Threads
// past the total write a count of 0, so the piece scan runs over max_spans.
__global__ __launch_bounds__(kFlThreads) void span_x_kernel(const ReadReq *__restrict__ req,
                                                            const uint64_t *__restrict__ rslot, uint64_t nreq,
                                                            const ReadPlan *__restrict__ plan,
                                                            const uint64_t *__restrict__ pstart,
                                                            const uint64_t *__restrict__ total_spans, ScrubView v,
                                                            SpanRec *recs, uint64_t *pcnt, uint64_t max_spans,
                                                            unsigned long long *touch) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t touched = 0;
    if (p < max_spans) {
        uint64_t cnt = 0;
        if (p < *total_spans) {
            uint64_t a = 0, b = nreq;  // last request r with pstart[r] <= p
            while (b - a > 1) {
                const uint64_t mid = (a + b) >> 1;
                if (pstart[mid] <= p) a = mid;
                else b = mid;
            }
            const ReadReq q = req[a];
            const ReadPlan pl = plan[a];
            const uint64_t k = p - pstart[a], i = pl.first + k;
            const uint64_t s0 = q.off[i], s1 = q.off[i + 1];
            const uint64_t from = s0 > pl.lo ? s0 : pl.lo, to = s1 < pl.hi ? s1 : pl.hi;
            const uint64_t len = to > from ? to - from : 0;
            if (q.spans) reinterpret_cast<cdc_chunk_pod *>(q.spans)[k] = cdc_chunk_pod{from - pl.lo, len};
            const uint32_t slot = reinterpret_cast<const uint32_t *>(rslot[a])[i];
            SpanRec r{s0, from, from + len, q.dst - pl.lo, ~0ull, slot, 0};
            if (slot != kNoSlot) {
                if (!v.kind[slot]) {
                    cnt = 1;
                } else {
                    touched = 1;
                    const uint64_t kf = v.key_first[slot], kc = v.key_count[slot];
                    if (kc && from == s0 && to == s1) {  // a whole span: every key
                        r.key0 = kf;
                        cnt = kc;
                    } else if (kc && len) {
                        // Only the two ends of a range: the keys that hold its first and last byte.
                        // Keys of length 0 share an offset with the key after them, so the last
                        // key starting at or before a byte is the one that holds it.
                        const uint64_t k0 = last_at_or_before(v.key_off, kf, kf + kc - 1, from - s0);
                        const uint64_t k1 = last_at_or_before(v.key_off, k0, kf + kc - 1, to - 1 - s0);
                        r.key0 = k0;
                        cnt = k1 - k0 + 1;
                    } else {
                        r.key0 = kf;
                    }
                }
            }
            recs[p] = r;
        }
        pcnt[p] = cnt;
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) touched += __shfl_xor(touched, k);
    if ((threadIdx.x & 63) == 0 && touched) atomicAdd(touch, (unsigned long long)touched);
}

__global__ __launch_bounds__(kFlThreads) void span_pieces_kernel(const SpanRec *__restrict__ recs,
                                                              const uint64_t *__restrict__ pstart,
                                                              uint64_t max_spans, ScrubView v,
                                                              const uint64_t *__restrict__ loc, uint64_t arena,
                                                              StorePiece *pieces, uint64_t *tiles,
                                                              uint64_t n_pieces) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pieces) return;
    uint64_t a = 0, b = max_spans;  // last span q with pstart[q] <= p (spans of no pieces share a start)
    while (b - a > 1) {
        const uint64_t mid = (a + b) >> 1;
        if (pstart[mid] <= p) a = mid;
        else b = mid;
    }
    const SpanRec r = recs[a];
    StorePiece pc;
    if (r.key0 == ~0ull) {
        pc.src = arena + loc[r.slot] + (r.from - r.s0);
        pc.dst = r.dst0 + r.from;
        pc.len = r.to - r.from;
    } else {
        const uint64_t k = r.key0 + (p - pstart[a]);
        const uint32_t ts = v.key_slot[k];
        const uint64_t k0 = r.s0 + v.key_off[k], k1 = k0 + v.t_length[ts];  // the key's bytes in the file
        const uint64_t from = k0 > r.from ? k0 : r.from, to = k1 < r.to ? k1 : r.to;
        pc.src = v.t_arena + v.t_loc[ts] + (from - k0);
        pc.dst = r.dst0 + from;
        pc.len = to > from ? to - from : 0;
    }
    pieces[p] = pc;
    tiles[p] = pc.len ? ((pc.dst & (kStoreAlign - 1)) + pc.len + (kStoreTile - 1)) / kStoreTile : 0;
}

// ---- distribution ----------------------------------------------------------------
__global__ __launch_bounds__(kFlThreads) void dist_init_kernel(const uint32_t *__restrict__ slot, uint64_t m,
                                                               uint32_t *cnt, uint64_t *firstpos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t s = slot[i];
    if (s == kNoSlot) return;
    cnt[s] = 0;  // every writer of a slot writes the same values
    firstpos[s] = ~0ull;
}

__global__ __launch_bounds__(kFlThreads) void dist_count_kernel(const uint32_t *__restrict__ slot, uint64_t m,
                                                                uint32_t *cnt, uint64_t *firstpos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t s = slot[i];
    if (s == kNoSlot) return;
    atomicAdd(&cnt[s], 1u);
    atomicMin((unsigned long long *)&firstpos[s], (unsigned long long)i);
}

__global__ __launch_bounds__(kFlThreads) void dist_flag_kernel(const uint32_t *__restrict__ slot, uint64_t m,
                                                               const uint64_t *__restrict__ firstpos, uint64_t *val) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t s = slot[i];
    val[i] = s != kNoSlot && firstpos[s] == i ? 1 : 0;
}

__global__ __launch_bounds__(kFlThreads) void dist_compact_kernel(SpanTable t, uint64_t m,
                                                                  const uint32_t *__restrict__ cnt,
                                                                  const uint64_t *__restrict__ firstpos,
                                                                  const uint64_t *__restrict__ val,
                                                                  const uint64_t *__restrict__ total, uint64_t cap,
                                                                  uint8_t *digests, uint32_t *counts,
                                                                  uint64_t *lengths) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || *total > cap) return;
    const uint32_t s = t.slot[i];
    if (s == kNoSlot || firstpos[s] != i) return;
    const uint64_t j = val[i];
    const uint4 *src = reinterpret_cast<const uint4 *>(t.digest + 32 * i);
    uint4 *dst = reinterpret_cast<uint4 *>(digests + 32 * j);
    dst[0] = src[0];
    dst[1] = src[1];
    counts[j] = cnt[s];
    lengths[j] = t.off[i + 1] - t.off[i];
}

// ---- get_to_dedup_ratio ------------------------------------------------------------
// The unique list of file_layer.rs:225-231 as span indices: the spans flagged as
// first occurrences by the distribution's kernels, at their rank val[i], with
// the length the reference gives them (the next span's offset minus their own).
__global__ __launch_bounds__(kFlThreads) void ratio_uniq_kernel(SpanTable t, uint64_t m,
                                                                const uint64_t *__restrict__ firstpos,
                                                                const uint64_t *__restrict__ val, uint64_t *uidx,
                                                                uint64_t *ulen) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t s = t.slot[i];
    if (s == kNoSlot || firstpos[s] != i) return;
    const uint64_t j = val[i];
    uidx[j] = i;
    ulen[j] = t.off[i + 1] - t.off[i];
}

// One thread.  pre = exclusive scan of the unique lengths over m entries (zero
// past the unique count), *pre_total their sum, so the sum of the first i
// lengths is pre[i] for i < m and *pre_total for i = m.  out[0] = C, the bytes
// of one cycle over the first R entries; out[1] = the largest i <= R whose
// prefix is <= total_size mod C: the entries the take-while accepts of the last,
// partial cycle (entries of length 0 count).  C = 0: out[1] = 0, the host refuses.
__global__ void ratio_take_kernel(const uint64_t *__restrict__ pre, const uint64_t *__restrict__ pre_total,
                                  uint64_t m, uint64_t R, uint64_t total_size, unsigned long long *out) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t C = R < m ? pre[R] : *pre_total;
    uint64_t lo = 0;
    if (C) {
        const uint64_t rem = total_size % C;
        uint64_t hi = R;  // prefix(0) = 0 <= rem
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            const uint64_t p = mid < m ? pre[mid] : *pre_total;
            if (p <= rem) lo = mid;
            else hi = mid - 1;
        }
    }
    out[0] = C;
    out[1] = lo;
}

// Output span i of the derived file takes unique entry i mod R while i < K (the
// repeating part) and R + i - K after it (the remaining entries): its source
// span goes to sidx, its length to the scan input, and the planner's bounds to
// stat as span_len_kernel leaves them.
__global__ __launch_bounds__(kFlThreads) void ratio_src_kernel(SpanTable src, const uint64_t *__restrict__ uidx,
                                                               uint64_t K, uint64_t R, uint64_t n, uint64_t *sidx,
                                                               uint64_t *val, unsigned long long *stat) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t least = ~0ull, zeros = 0;
    if (i < n) {
        const uint64_t si = uidx[i < K ? i % R : R + (i - K)];
        const uint64_t len = src.off[si + 1] - src.off[si];
        sidx[i] = si;
        val[i] = len;
        least = len - 1;
        zeros = len == 0;
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const uint64_t o = __shfl_xor(least, k);
        least = o < least ? o : least;
        zeros += __shfl_xor(zeros, k);
    }
    if ((threadIdx.x & 63) == 0) {
        if (least != ~0ull) atomicMin(&stat[0], (unsigned long long)least);
        if (zeros) atomicAdd(&stat[1], (unsigned long long)zeros);
    }
}

// val = exclusive scan of the lengths: the true offsets in the new file.
__global__ __launch_bounds__(kFlThreads) void ratio_write_kernel(SpanTable src, SpanTable dst,
                                                                 const uint64_t *__restrict__ sidx,
                                                                 const uint64_t *__restrict__ val,
                                                                 const uint64_t *__restrict__ total, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        dst.off[n] = *total;
        return;
    }
    const uint64_t si = sidx[i];
    dst.off[i] = val[i];
    dst.slot[i] = src.slot[si];
    dst.loc[i] = src.loc[si];
    const uint4 *from = reinterpret_cast<const uint4 *>(src.digest + 32 * si);
    uint4 *to = reinterpret_cast<uint4 *>(dst.digest + 32 * i);
    to[0] = from[0];
    to[1] = from[1];
}

// ---- splice (cdc_file_splice_device) -----------------------------------------------
// One thread: the start span and its offset.
__global__ void splice_start_kernel(const uint64_t *__restrict__ off, uint64_t n, uint64_t offset,
                                    unsigned long long *out) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t i0 = splice_start_span(off, n, offset);
    out[0] = i0;
    out[1] = off[i0];
}

// Whether chunk k of the window resyncs: it is trusted, its cut lies at or past
// the inserted bytes and, moved back by delta, on an old boundary (*j, the first
// of equal offsets).
__device__ __forceinline__ bool splice_meets(const cdc_chunk_pod c, const SpliceRound &r,
                                             const uint64_t *__restrict__ off, uint64_t n, uint64_t *e, uint64_t *j) {
    const uint64_t start = r.w0 + c.offset;
    *e = start + c.length;
    if (!splice_trusted(start, r.max_chunk, r.end_w, r.size_after)) return false;
    if (*e < r.offset + r.insert_len) return false;
    return splice_old_boundary(off, n, *e, r.remove_len, r.insert_len, j);
}

// One thread per new chunk; the smallest k that meets, reduced within the wave,
// then one atomicMin per wave.
__global__ __launch_bounds__(kFlThreads) void splice_resync_kernel(const cdc_chunk_pod *__restrict__ chunks,
                                                                   uint64_t m, SpliceRound r,
                                                                   const uint64_t *__restrict__ off, uint64_t n,
                                                                   unsigned long long *best) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t cand = ~0ull;
    if (k < m) {
        uint64_t e, j;
        if (splice_meets(chunks[k], r, off, n, &e, &j)) cand = k;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_xor(cand, d);
        cand = o < cand ? o : cand;
    }
    if ((threadIdx.x & 63) == 0 && cand != ~0ull) atomicMin(best, (unsigned long long)cand);
}

// One thread: {k, j, e_k} of the winner for the host.
__global__ void splice_pick_kernel(const cdc_chunk_pod *__restrict__ chunks, SpliceRound r,
                                   const uint64_t *__restrict__ off, uint64_t n,
                                   const unsigned long long *__restrict__ best, unsigned long long *out) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t k = *best;
    uint64_t e = 0, j = 0;
    if (k != ~0ull) (void)splice_meets(chunks[k], r, off, n, &e, &j);
    out[0] = k;
    out[1] = j;
    out[2] = e;
}

// val = exclusive scan of the m accepted lengths.  Entry t of the new table:
// t < i0 the old entry; t < i0 + m accepted chunk t - i0, as append_kernel writes
// it; after that old entry j + (t - i0 - m) with its offset moved.  Entry n_new
// closes the table.  patch: dst is the old table, only [i0, i0 + m) is written
// (the offsets around it stay what they are).
__global__ __launch_bounds__(kFlThreads) void splice_build_kernel(SpanTable old, SpanTable dst, uint64_t i0,
                                                                  uint64_t j, uint64_t n, uint64_t size_old,
                                                                  uint64_t w0, uint64_t rem, uint64_t ins,
                                                                  uint64_t n_new, bool patch,
                                                                  const uint32_t *__restrict__ slot_of,
                                                                  const uint64_t *__restrict__ tbl_loc,
                                                                  const uint8_t *__restrict__ digests, uint64_t m,
                                                                  const uint64_t *__restrict__ val) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (patch) {
        if (t >= m) return;
        t += i0;
    } else if (t > n_new) {
        return;
    }
    if (t >= i0 && t < i0 + m) {
        const uint64_t c = t - i0;
        const uint32_t s = slot_of[c];
        dst.off[t] = w0 + val[c];
        dst.slot[t] = s;
        dst.loc[t] = s == kNoSlot ? 0 : tbl_loc[s];
        const uint4 *src = reinterpret_cast<const uint4 *>(digests + 32 * c);
        uint4 *to = reinterpret_cast<uint4 *>(dst.digest + 32 * t);
        to[0] = src[0];
        to[1] = src[1];
        return;
    }
    const uint64_t si = t < i0 ? t : j + (t - i0 - m);
    const uint64_t o = si == n ? size_old : old.off[si];  // a file without spans has no table
    dst.off[t] = t < i0 ? o : o - rem + ins;
    if (t == n_new) return;
    dst.slot[t] = old.slot[si];
    dst.loc[t] = old.loc[si];
    const uint4 *src = reinterpret_cast<const uint4 *>(old.digest + 32 * si);
    uint4 *to = reinterpret_cast<uint4 *>(dst.digest + 32 * t);
    to[0] = src[0];
    to[1] = src[1];
}

// ---- collect (cdc_files_collect) --------------------------------------------------
// The m spans of all the layer's files in one launch, segmented as the batch
// append is: span i belongs to file f = file_of_span(first, nfiles, i).
// refs[slot] += 1 per span.  A wave first combines: for up to kRefRounds
// leaders, the lanes that name the leader's slot retire with one atomic of their
// count (a file that repeats one chunk would otherwise serialise on one
// address); what is left after that -- a wave of mostly distinct slots -- adds
// for itself.
constexpr int kRefRounds = 4;

__global__ __launch_bounds__(kFlThreads) void collect_refs_kernel(const CollectSeg *__restrict__ seg,
                                                                  const uint64_t *__restrict__ first, uint64_t nfiles,
                                                                  uint64_t m, uint64_t slots,
                                                                  unsigned long long *refs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool todo = false;
    uint32_t s = kNoSlot;
    if (i < m) {
        const uint64_t f = file_of_span(first, nfiles, i);
        s = seg[f].slot[i - first[f]];
        todo = s < slots;  // 0xFFFFFFFF: a span without a slot
    }
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long left = __ballot(todo);
    for (int round = 0; round < kRefRounds && left; ++round) {  // wave-uniform
        const uint32_t leader = (uint32_t)__builtin_ctzll(left);
        const uint32_t lead_slot = __shfl(s, (int)leader);
        const bool mine = todo && s == lead_slot;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&refs[lead_slot], (unsigned long long)__popcll(same));
        if (mine) todo = false;
        left &= ~same;
    }
    if (todo) atomicAdd(&refs[s], 1ull);
}

// After the store's collect: every span's slot through map (old slot -> new
// slot) and its arena offset from the new table.
__global__ __launch_bounds__(kFlThreads) void collect_remap_kernel(const CollectSeg *__restrict__ seg,
                                                                   const uint64_t *__restrict__ first, uint64_t nfiles,
                                                                   uint64_t m, uint64_t slots,
                                                                   const uint32_t *__restrict__ map,
                                                                   const uint64_t *__restrict__ new_loc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t f = file_of_span(first, nfiles, i), j = i - first[f];
    const CollectSeg sg = seg[f];
    const uint32_t s = sg.slot[j];
    if (s >= slots) return;
    const uint32_t ns = map[s];  // referenced, so it survived
    if (ns == kNoSlot) return;
    sg.slot[j] = ns;
    sg.loc[j] = new_loc[ns];
}

// ---- diff ---------------------------------------------------------------------------
static_assert(kDiffTile == kStoreTile && kDiffAlign == kStoreAlign, "diff_plan.hpp cuts the store's tiles");
static_assert(kReadTile == kStoreTile && kReadAlign == kStoreAlign, "read_plan.hpp bounds the store's tiles");
constexpr int kFlWaves = kFlThreads / 64;
constexpr unsigned kDiffMaxBlocks = 1u << 18;  // waves (threads of the fix-up) past this stride

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) v += __shfl_xor(v, k);
    return v;
}
// Exclusive prefix sum over the wave.
__device__ __forceinline__ uint32_t wave_excl(uint32_t v, uint32_t lane) {
    uint32_t inc = v;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const uint32_t o = __shfl_up(inc, k);
        if (lane >= (uint32_t)k) inc += o;
    }
    return inc - v;
}

// Stage 1a: one thread per span boundary of either table.
__global__ __launch_bounds__(kFlThreads) void diff_flag_kernel(DiffSide a, DiffSide b, uint64_t common, uint64_t nc,
                                                               uint64_t *cand) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    uint64_t x;
    cand[c] = diff_opens(a.off, a.n, b.off, b.n, common, c, &x) ? 1 : 0;
}

// Stage 1b, after the scan: the merge by ranking.
__global__ __launch_bounds__(kFlThreads) void diff_piece_kernel(DiffSide a, DiffSide b, uint64_t common, uint64_t nc,
                                                                const uint64_t *__restrict__ cand, uint64_t *pstart,
                                                                uint32_t *pia, uint32_t *pib) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    uint64_t x;
    if (!diff_opens(a.off, a.n, b.off, b.n, common, c, &x)) return;
    uint32_t ia, ib;
    const uint64_t p = diff_rank(a.off, a.n, b.off, b.n, cand, c, x, &ia, &ib);
    pstart[p] = x;
    pia[p] = ia;
    pib[p] = ib;
}

__device__ __forceinline__ bool piece_shared(const DiffSide &a, const DiffSide &b, const uint32_t *__restrict__ pia,
                                             const uint32_t *__restrict__ pib, uint64_t p) {
    const uint32_t ia = pia[p], ib = pib[p];
    return diff_shared(a.slot[ia], a.off[ia], b.slot[ib], b.off[ib]);
}

// Stage 2a: the sharing rule.  pflag = the piece is compared (exact), or it
// begins a run of pieces that are not shared (tables only); acc[0] += the bytes
// of the pieces that are not shared.  Threads past the piece count write 0, so
// the scan runs over max_pieces.
__global__ __launch_bounds__(kFlThreads) void diff_share_kernel(DiffSide a, DiffSide b, uint64_t common,
                                                                const uint64_t *__restrict__ n_pieces,
                                                                const uint64_t *__restrict__ pstart,
                                                                const uint32_t *__restrict__ pia,
                                                                const uint32_t *__restrict__ pib, uint64_t max_pieces,
                                                                bool tables_only, uint64_t *pflag,
                                                                unsigned long long *acc) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t P = *n_pieces;
    uint64_t bytes = 0, flag = 0;
    if (p < P && !piece_shared(a, b, pia, pib, p)) {
        bytes = (p + 1 < P ? pstart[p + 1] : common) - pstart[p];
        flag = !tables_only || p == 0 || piece_shared(a, b, pia, pib, p - 1);
    }
    if (p < max_pieces) pflag[p] = flag;
    bytes = wave_sum(bytes);
    if ((threadIdx.x & 63) == 0 && bytes) atomicAdd(&acc[0], (unsigned long long)bytes);
}

// Stage 2b (exact): the compared pieces, compacted.  Entries from the compared
// count on are written empty, so the tile scan runs over max_pieces.
__global__ __launch_bounds__(kFlThreads) void diff_compact_kernel(DiffSide a, DiffSide b, uint64_t common,
                                                                  uint64_t arena, DiffScratch w) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.max_pieces) return;
    const uint64_t P = *w.n_pieces;
    const uint64_t C = *w.n_cmp;
    if (p >= C) {
        w.cp[p] = StorePiece{0, 0, 0};
        w.tstart[p] = 0;
    }
    if (p >= P || piece_shared(a, b, w.pia, w.pib, p)) return;
    const uint64_t c = w.pflag[p], x = w.pstart[p], end = p + 1 < P ? w.pstart[p + 1] : common;
    const uint32_t ia = w.pia[p], ib = w.pib[p];
    const StorePiece pc{arena + a.loc[ia] + (x - a.off[ia]), arena + b.loc[ib] + (x - b.off[ib]), end - x};
    w.cp[c] = pc;
    w.tstart[c] = diff_tiles(pc.dst, pc.len);
    w.cx[c] = x;
    w.cflag[c] = (p > 0 && !piece_shared(a, b, w.pia, w.pib, p - 1) ? 1u : 0u) |
                 (end == common && a.size != b.size ? 2u : 0u);
}

__device__ __forceinline__ uint64_t mask_bit(const uint64_t *__restrict__ mask, uint64_t tile, uint32_t b) {
    return (mask[tile * kDiffTileWords + b / 64] >> (b % 64)) & 1;
}
// Does the last byte of compared piece c differ?
__device__ __forceinline__ uint64_t last_bit_of(const DiffScratch &w, uint64_t c) {
    uint64_t k;
    uint32_t b;
    diff_last_bit((uint32_t)(w.cp[c].dst & (kDiffAlign - 1)), w.cp[c].len, &k, &b);
    return mask_bit(w.mask, w.tstart[c] + k, b);
}

// Tile T of the tile scan as the run passes see it; *x = its piece's first byte
// in the file.  The same in every lane.
__device__ __forceinline__ DiffTile diff_tile_at(const DiffScratch &w, uint64_t C, uint64_t T, uint64_t *x) {
    uint64_t lo = 0, hi = w.max_pieces;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (w.tstart[mid] <= T) lo = mid;
        else hi = mid;
    }
    const uint64_t c = lo;
    const StorePiece pc = w.cp[c];
    DiffTile t;
    t.m = (uint32_t)(pc.dst & (kDiffAlign - 1));
    t.len = pc.len;
    t.k = T - w.tstart[c];
    t.head_joined = t.k == 0 && (w.cflag[c] & 1u) && last_bit_of(w, c - 1);
    t.tail_joined = false;
    if (t.k + 1 == diff_tiles(pc.dst, pc.len))
        t.tail_joined = (w.cflag[c] & 2u) ||
                        (c + 1 < C && (w.cflag[c + 1] & 1u) &&
                         mask_bit(w.mask, w.tstart[c + 1], (uint32_t)(w.cp[c + 1].dst & (kDiffAlign - 1))));
    *x = w.cx[c];
    return t;
}

// Stage 4a: one wave per tile, one lane per mask word.  tcount[T] = the runs
// that begin in tile T (0 from the tile total on, so the scan runs over
// max_tiles); acc[1] += the set bits.
__global__ __launch_bounds__(kFlThreads) void diff_count_kernel(DiffScratch w) {
    const uint64_t TT = *w.n_tiles, C = *w.n_cmp;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kFlWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * kFlWaves;
    for (uint64_t T = wave0; T < w.max_tiles; T += nwaves) {
        if (T >= TT) {
            if (lane == 0) w.tcount[T] = 0;
            continue;
        }
        uint64_t x;
        const DiffTile t = diff_tile_at(w, C, T, &x);
        const uint64_t word = w.mask[T * kDiffTileWords + lane];
        uint64_t prev = __shfl_up(word, 1) >> 63;
        if (lane == 0) prev = t.k ? w.mask[T * kDiffTileWords - 1] >> 63 : 0;
        const uint64_t starts = wave_sum((uint64_t)__popcll(diff_tile_starts(t, lane, word, prev)));
        const uint64_t bits = wave_sum((uint64_t)__popcll(word));
        if (lane == 0) {
            w.tcount[T] = starts;
            if (bits) atomicAdd(&w.acc[1], (unsigned long long)bits);
        }
    }
}

// The count of the whole answer and the stats, by one thread after the last
// scan.  S = runs that begin below `common`.
__global__ void diff_total_kernel(DiffSide a, DiffSide b, uint64_t common, bool tables_only, DiffScratch w,
                                  unsigned long long *h_out) {
    const uint64_t P = *w.n_pieces;
    const uint64_t C = *w.n_cmp;  // tables only: S
    const bool tail = a.size != b.size;
    const uint64_t maxsz = a.size > b.size ? a.size : b.size;
    uint64_t S, joined = 0, differing;
    if (tables_only) {
        S = C;
        joined = tail && P && !piece_shared(a, b, w.pia, w.pib, P - 1);
        differing = w.acc[0];
    } else {
        S = *w.n_starts;
        joined = tail && C && (w.cflag[C - 1] & 2u) && last_bit_of(w, C - 1);
        differing = w.acc[1];
    }
    const uint64_t R = S + (tail && !joined ? 1 : 0);
    w.acc[2] = R;
    w.acc[3] = joined;
    h_out[0] = R;
    h_out[1] = differing + (maxsz - common);
    h_out[2] = tables_only ? 0 : w.acc[0];
    h_out[3] = common - w.acc[0];
    h_out[4] = P;
}

// The tail [common, max): a range of its own, or the end of the run it continues.
__device__ __forceinline__ void diff_emit_tail(const DiffSide &a, const DiffSide &b, uint64_t common,
                                               const unsigned long long *acc, cdc_chunk_pod *ranges) {
    if (a.size == b.size) return;
    const uint64_t R = acc[2], maxsz = a.size > b.size ? a.size : b.size;
    if (acc[3]) ranges[R - 1].length = maxsz;
    else ranges[R - 1] = cdc_chunk_pod{common, maxsz};
}

// Stage 4b (exact): run r gets its first byte from the thread that holds its
// start bit and, in `length`, its END from the thread that holds its end bit;
// diff_fix_kernel turns ends into lengths.  Nothing is written when the count
// exceeds cap.
__global__ __launch_bounds__(kFlThreads) void diff_emit_kernel(DiffSide a, DiffSide b, uint64_t common, DiffScratch w,
                                                               cdc_chunk_pod *ranges, uint64_t cap) {
    if (w.acc[2] > cap) return;
    const uint64_t TT = *w.n_tiles, C = *w.n_cmp;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * kFlWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * kFlWaves;
    if (blockIdx.x == 0 && threadIdx.x == 0) diff_emit_tail(a, b, common, w.acc, ranges);
    for (uint64_t T = wave0; T < TT; T += nwaves) {
        uint64_t x;
        const DiffTile t = diff_tile_at(w, C, T, &x);
        const uint64_t word = w.mask[T * kDiffTileWords + lane];
        uint64_t prev = __shfl_up(word, 1) >> 63, next = __shfl_down(word, 1) & 1;
        if (lane == 0) prev = t.k ? w.mask[T * kDiffTileWords - 1] >> 63 : 0;
        if (lane == 63) next = t.k + 1 < diff_tiles(t.m, t.len) ? w.mask[(T + 1) * kDiffTileWords] & 1 : 0;
        uint64_t starts = diff_tile_starts(t, lane, word, prev), ends = diff_tile_ends(t, lane, word, next);
        const uint64_t open = __shfl(lane == 0 ? diff_tile_open(t, word, starts) : 0, 0);
        uint64_t rs = w.tcount[T] + wave_excl((uint32_t)__popcll(starts), lane);
        uint64_t re = w.tcount[T] - open + wave_excl((uint32_t)__popcll(ends), lane);
        for (; starts; starts &= starts - 1)
            ranges[rs++].offset = diff_file_offset(x, t.m, t.k, lane * 64 + (uint32_t)__builtin_ctzll(starts));
        for (; ends; ends &= ends - 1)
            ranges[re++].length = diff_file_offset(x, t.m, t.k, lane * 64 + (uint32_t)__builtin_ctzll(ends)) + 1;
    }
}

// The same for CDC_DIFF_TABLES_ONLY: the runs of pieces that are not shared.
__global__ __launch_bounds__(kFlThreads) void diff_emit_tables_kernel(DiffSide a, DiffSide b, uint64_t common,
                                                                      DiffScratch w, cdc_chunk_pod *ranges,
                                                                      uint64_t cap) {
    if (w.acc[2] > cap) return;
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) diff_emit_tail(a, b, common, w.acc, ranges);
    const uint64_t P = *w.n_pieces;
    if (p >= P || piece_shared(a, b, w.pia, w.pib, p)) return;
    const bool start = p == 0 || piece_shared(a, b, w.pia, w.pib, p - 1);
    const bool end = p + 1 < P ? piece_shared(a, b, w.pia, w.pib, p + 1) : a.size == b.size;
    const uint64_t r = w.pflag[p];  // runs that begin before piece p
    if (start) ranges[r].offset = w.pstart[p];
    if (end) ranges[r + (start ? 1 : 0) - 1].length = p + 1 < P ? w.pstart[p + 1] : common;
}

__global__ __launch_bounds__(kFlThreads) void diff_fix_kernel(const unsigned long long *__restrict__ acc,
                                                              cdc_chunk_pod *ranges, uint64_t cap) {
    const uint64_t R = acc[2];
    if (R > cap) return;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (uint64_t)gridDim.x * blockDim.x)
        ranges[r].length -= ranges[r].offset;
}

}  // namespace

hipError_t launch_splice_start(const uint64_t *off, uint64_t n, uint64_t offset, unsigned long long *h_out,
                               hipStream_t s) {
    splice_start_kernel<<<1, 64, 0, s>>>(off, n, offset, h_out);
    return hipGetLastError();
}

hipError_t launch_splice_resync(const cdc_chunk_pod *chunks, uint64_t m, const SpliceRound &r, const uint64_t *off,
                                uint64_t n, unsigned long long *d_best, unsigned long long *h_out, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(d_best, 0xFF, 8, s);
    if (e != hipSuccess) return e;
    splice_resync_kernel<<<grid_of(m), kFlThreads, 0, s>>>(chunks, m, r, off, n, d_best);
    splice_pick_kernel<<<1, 64, 0, s>>>(chunks, r, off, n, d_best, h_out);
    return hipGetLastError();
}

hipError_t launch_splice_build(const SpanTable &old, uint64_t n, uint64_t size_old, const SpanTable &dst,
                               uint64_t i0, uint64_t j, uint64_t w0, uint64_t rem, uint64_t ins, const uint32_t *slot_of,
                               const uint64_t *tbl_length, const uint64_t *tbl_loc, const uint8_t *d_digests,
                               uint64_t m, uint64_t *val, uint64_t *block_sums, unsigned long long *d_stat,
                               unsigned long long *h_total, hipStream_t s) {
    span_len_kernel<<<grid_of(m), kFlThreads, 0, s>>>(slot_of, tbl_length, m, val, d_stat);
    const hipError_t e = launch_store_scan(val, m, block_sums, h_total, s);
    if (e != hipSuccess) return e;
    const uint64_t n_new = i0 + m + (n - j);
    const bool patch = dst.off == old.off;
    splice_build_kernel<<<grid_of(patch ? m : n_new + 1), kFlThreads, 0, s>>>(
        old, dst, i0, j, n, size_old, w0, rem, ins, n_new, patch, slot_of, tbl_loc, d_digests, m, val);
    return hipGetLastError();
}

hipError_t launch_files_refs(const CollectSeg *d_seg, const uint64_t *d_first, uint64_t nfiles, uint64_t m,
                             uint64_t slots, unsigned long long *refs, hipStream_t s) {
    if (!m) return hipSuccess;
    collect_refs_kernel<<<grid_of(m), kFlThreads, 0, s>>>(d_seg, d_first, nfiles, m, slots, refs);
    return hipGetLastError();
}

hipError_t launch_files_remap(const CollectSeg *d_seg, const uint64_t *d_first, uint64_t nfiles, uint64_t m,
                              uint64_t slots, const uint32_t *map, const uint64_t *new_loc, hipStream_t s) {
    if (!m) return hipSuccess;
    collect_remap_kernel<<<grid_of(m), kFlThreads, 0, s>>>(d_seg, d_first, nfiles, m, slots, map, new_loc);
    return hipGetLastError();
}

hipError_t launch_files_diff(const DiffSide &a, const DiffSide &b, uint64_t arena, bool tables_only,
                             const DiffScratch &w, cdc_chunk_pod *d_ranges, uint64_t cap, unsigned long long *h_out,
                             hipStream_t s) {
    const uint64_t common = a.size < b.size ? a.size : b.size, maxsz = a.size < b.size ? b.size : a.size;
    const uint64_t nc = diff_candidates(a.n, b.n), mp = w.max_pieces;
    hipError_t e = hipMemsetAsync(w.acc, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    // 1. Ranks: the pieces in file order.
    diff_flag_kernel<<<grid_of(nc), kFlThreads, 0, s>>>(a, b, common, nc, w.cand);
    if ((e = launch_store_scan(w.cand, nc, w.bs_c, nullptr, s)) != hipSuccess) return e;
    diff_piece_kernel<<<grid_of(nc), kFlThreads, 0, s>>>(a, b, common, nc, w.cand, w.pstart, w.pia, w.pib);
    // 2. The sharing rule, and the compared pieces as a piece list.
    diff_share_kernel<<<grid_of(mp), kFlThreads, 0, s>>>(a, b, common, w.n_pieces, w.pstart, w.pia, w.pib, mp,
                                                         tables_only, w.pflag, w.acc);
    if ((e = launch_store_scan(w.pflag, mp, w.bs_p, nullptr, s)) != hipSuccess) return e;
    // A run holds a byte or more: the count is at most half the bytes, rounded up.
    const uint64_t most = maxsz / 2 + 1, fix = cap < most ? cap : most;
    const uint64_t fix_blocks = (fix + kFlThreads - 1) / kFlThreads;
    const unsigned fix_grid = (unsigned)(fix_blocks < kDiffMaxBlocks ? fix_blocks : kDiffMaxBlocks);
    if (tables_only) {
        diff_total_kernel<<<1, 1, 0, s>>>(a, b, common, true, w, h_out);
        if (!cap) return hipGetLastError();
        diff_emit_tables_kernel<<<grid_of(mp), kFlThreads, 0, s>>>(a, b, common, w, d_ranges, cap);
        diff_fix_kernel<<<fix_grid, kFlThreads, 0, s>>>(w.acc, d_ranges, cap);
        return hipGetLastError();
    }
    diff_compact_kernel<<<grid_of(mp), kFlThreads, 0, s>>>(a, b, common, arena, w);
    if ((e = launch_store_scan(w.tstart, mp, w.bs_t, nullptr, s)) != hipSuccess) return e;
    // 3. One bit per compared byte.
    if ((e = launch_store_diff_mask(w.cp, w.tstart, mp, w.max_tiles, w.n_tiles, w.mask, s)) !=
        hipSuccess)
        return e;
    // 4. Runs: starts per tile, their scan, the emit.
    const uint64_t blocks = (w.max_tiles + kFlWaves - 1) / kFlWaves;
    const unsigned tile_grid = (unsigned)(blocks < kDiffMaxBlocks ? blocks : kDiffMaxBlocks);
    diff_count_kernel<<<tile_grid, kFlThreads, 0, s>>>(w);
    if ((e = launch_store_scan(w.tcount, w.max_tiles, w.bs_r, nullptr, s)) != hipSuccess) return e;
    diff_total_kernel<<<1, 1, 0, s>>>(a, b, common, false, w, h_out);
    if (!cap) return hipGetLastError();
    diff_emit_kernel<<<tile_grid, kFlThreads, 0, s>>>(a, b, common, w, d_ranges, cap);
    diff_fix_kernel<<<fix_grid, kFlThreads, 0, s>>>(w.acc, d_ranges, cap);
    return hipGetLastError();
}

hipError_t launch_files_ratio_unique(const SpanTable &t, uint64_t m, uint32_t *cnt, uint64_t *firstpos, uint64_t *val,
                                     uint64_t *block_sums, uint64_t *uidx, uint64_t *ulen, uint64_t *ublock,
                                     unsigned long long *h_out, hipStream_t s) {
    if (!m) return hipSuccess;
    dist_init_kernel<<<grid_of(m), kFlThreads, 0, s>>>(t.slot, m, cnt, firstpos);
    dist_count_kernel<<<grid_of(m), kFlThreads, 0, s>>>(t.slot, m, cnt, firstpos);
    dist_flag_kernel<<<grid_of(m), kFlThreads, 0, s>>>(t.slot, m, firstpos, val);
    hipError_t e = launch_store_scan(val, m, block_sums, h_out, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(ulen, 0, m * 8, s);
    if (e != hipSuccess) return e;
    ratio_uniq_kernel<<<grid_of(m), kFlThreads, 0, s>>>(t, m, firstpos, val, uidx, ulen);
    return launch_store_scan(ulen, m, ublock, h_out + 1, s);
}

hipError_t launch_files_ratio_take(const uint64_t *pre, const uint64_t *ublock, uint64_t m, uint64_t R,
                                   uint64_t total_size, unsigned long long *h_out, hipStream_t s) {
    ratio_take_kernel<<<1, 64, 0, s>>>(pre, ublock + store_scan_blocks(m), m, R, total_size, h_out);
    return hipGetLastError();
}

hipError_t launch_files_ratio_gather(const SpanTable &src, const SpanTable &dst, const uint64_t *uidx, uint64_t K,
                                     uint64_t R, uint64_t n, uint64_t *sidx, uint64_t *val, uint64_t *block_sums,
                                     unsigned long long *d_stat, unsigned long long *h_total, hipStream_t s) {
    if (!n) return hipSuccess;
    ratio_src_kernel<<<grid_of(n), kFlThreads, 0, s>>>(src, uidx, K, R, n, sidx, val, d_stat);
    const hipError_t e = launch_store_scan(val, n, block_sums, h_total, s);
    if (e != hipSuccess) return e;
    ratio_write_kernel<<<grid_of(n + 1), kFlThreads, 0, s>>>(src, dst, sidx, val, block_sums + store_scan_blocks(n), n);
    return hipGetLastError();
}

hipError_t launch_files_append(const SpanTable &t, uint64_t n0, uint64_t size0, const uint32_t *slot_of,
                               const uint64_t *tbl_length, const uint64_t *tbl_loc, const uint8_t *d_digests,
                               uint64_t n, uint64_t *val, uint64_t *block_sums, unsigned long long *d_stat,
                               unsigned long long *h_total, hipStream_t s) {
    if (!n) return hipSuccess;
    span_len_kernel<<<grid_of(n), kFlThreads, 0, s>>>(slot_of, tbl_length, n, val, d_stat);
    hipError_t e = launch_store_scan(val, n, block_sums, h_total, s);
    if (e != hipSuccess) return e;
    append_kernel<<<grid_of(n + 1), kFlThreads, 0, s>>>(t, n0, size0, slot_of, tbl_loc, d_digests, n, val,
                                                        block_sums + store_scan_blocks(n));
    return hipGetLastError();
}

hipError_t launch_files_append_batch(const AppendDst *d_dst, const uint64_t *d_first, uint64_t nfiles, uint64_t m,
                                     const uint32_t *slot_of, const uint64_t *tbl_length, const uint64_t *tbl_loc,
                                     const uint8_t *d_digests, uint64_t *val, uint64_t *block_sums,
                                     AppendStat *d_stat, hipStream_t s) {
    if (!m) return hipSuccess;
    batch_len_kernel<<<grid_of(m), kFlThreads, 0, s>>>(slot_of, tbl_length, d_first, nfiles, m, val, d_stat);
    const hipError_t e = launch_store_scan(val, m, block_sums, nullptr, s);
    if (e != hipSuccess) return e;
    batch_append_kernel<<<grid_of(m + nfiles), kFlThreads, 0, s>>>(d_dst, d_first, nfiles, m, slot_of, tbl_loc,
                                                                   d_digests, val, block_sums + store_scan_blocks(m),
                                                                   d_stat);
    return hipGetLastError();
}

hipError_t launch_files_read(const ReadReq *d_req, uint64_t nreq, uint64_t arena, ReadPlan *plan, uint64_t *cnt,
                             uint64_t *rblock, StorePiece *pieces, uint64_t *tstart, uint64_t *block_sums,
                             uint64_t max_pieces, uint64_t max_tiles, ReadResult *h_res, hipStream_t s,
                             uint64_t cmp_base, unsigned long long *d_diff) {
    if (!nreq) return hipSuccess;
    uint64_t *total_pieces = rblock + store_scan_blocks(nreq);
    resolve_kernel<<<grid_of(nreq), kFlThreads, 0, s>>>(d_req, nreq, plan, cnt, nreq == 1 ? total_pieces : nullptr,
                                                        h_res);
    if (!max_pieces) return hipGetLastError();
    hipError_t e = nreq == 1 ? hipSuccess : launch_store_scan(cnt, nreq, rblock, nullptr, s);
    if (e != hipSuccess) return e;
    pieces_kernel<<<grid_of(max_pieces), kFlThreads, 0, s>>>(d_req, nreq, plan, cnt, total_pieces, arena, pieces,
                                                             tstart, max_pieces);
    e = launch_store_scan(tstart, max_pieces, block_sums, nullptr, s);
    if (e != hipSuccess) return e;
    if (d_diff)
        return launch_store_compare(pieces, tstart, max_pieces, max_tiles, block_sums + store_scan_blocks(max_pieces),
                                    cmp_base, d_diff, s);
    return launch_store_copy(pieces, tstart, max_pieces, max_tiles, block_sums + store_scan_blocks(max_pieces), s);
}

hipError_t launch_files_plan_x(const ReadReq *d_req, const uint64_t *d_rslot, uint64_t nreq, const ScrubView &v,
                               ReadPlan *plan, uint64_t *cnt, uint64_t *rblock, SpanRec *recs, uint64_t *pcnt,
                               uint64_t *pblock, uint64_t max_spans, ReadResult *h_res,
                               unsigned long long *d_touch, unsigned long long *h_tot, hipStream_t s) {
    if (!nreq) return hipSuccess;
    uint64_t *total_spans = rblock + store_scan_blocks(nreq);
    resolve_kernel<<<grid_of(nreq), kFlThreads, 0, s>>>(d_req, nreq, plan, cnt, nreq == 1 ? total_spans : nullptr,
                                                        h_res);
    h_tot[0] = h_tot[1] = 0;
    if (!max_spans) return hipGetLastError();
    hipError_t e = nreq == 1 ? hipSuccess : launch_store_scan(cnt, nreq, rblock, nullptr, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d_touch, 0, 8, s);
    if (e != hipSuccess) return e;
    span_x_kernel<<<grid_of(max_spans), kFlThreads, 0, s>>>(d_req, d_rslot, nreq, plan, cnt, total_spans, v, recs,
                                                            pcnt, max_spans, d_touch);
    e = launch_store_scan(pcnt, max_spans, pblock, h_tot, s);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(h_tot + 1, d_touch, 8, hipMemcpyDeviceToHost, s);
}

hipError_t launch_files_copy_x(const SpanRec *recs, const uint64_t *pcnt, uint64_t max_spans, const ScrubView &v,
                               const uint64_t *loc, uint64_t arena, StorePiece *pieces, uint64_t *tstart,
                               uint64_t *block_sums, uint64_t n_pieces, uint64_t max_tiles, hipStream_t s,
                               uint64_t cmp_base, unsigned long long *d_diff) {
    if (!n_pieces) return hipSuccess;
    span_pieces_kernel<<<grid_of(n_pieces), kFlThreads, 0, s>>>(recs, pcnt, max_spans, v, loc, arena, pieces, tstart,
                                                             n_pieces);
    const hipError_t e = launch_store_scan(tstart, n_pieces, block_sums, nullptr, s);
    if (e != hipSuccess) return e;
    if (d_diff)
        return launch_store_compare(pieces, tstart, n_pieces, max_tiles, block_sums + store_scan_blocks(n_pieces),
                                    cmp_base, d_diff, s);
    return launch_store_copy(pieces, tstart, n_pieces, max_tiles, block_sums + store_scan_blocks(n_pieces), s);
}

hipError_t launch_files_distribution(const SpanTable &t, uint64_t m, uint32_t *cnt, uint64_t *firstpos,
                                     uint64_t *val, uint64_t *block_sums, uint8_t *d_digests, uint32_t *d_counts,
                                     uint64_t *d_lengths, uint64_t cap, unsigned long long *h_distinct,
                                     hipStream_t s) {
    if (!m) return hipSuccess;
    dist_init_kernel<<<grid_of(m), kFlThreads, 0, s>>>(t.slot, m, cnt, firstpos);
    dist_count_kernel<<<grid_of(m), kFlThreads, 0, s>>>(t.slot, m, cnt, firstpos);
    dist_flag_kernel<<<grid_of(m), kFlThreads, 0, s>>>(t.slot, m, firstpos, val);
    hipError_t e = launch_store_scan(val, m, block_sums, h_distinct, s);
    if (e != hipSuccess) return e;
    dist_compact_kernel<<<grid_of(m), kFlThreads, 0, s>>>(t, m, cnt, firstpos, val, block_sums + store_scan_blocks(m),
                                                          cap, d_digests, d_counts, d_lengths);
    return hipGetLastError();
}

}  // namespace cdc
