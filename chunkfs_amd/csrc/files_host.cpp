// files_host.cpp -- C ABI of the device file layer (include/chunkfs_amd.h, "File
// layer"): the reference's FileLayer (src/system/file_layer.rs) and the
// FileSystem calls built on it (src/system/mod.rs:58-160, 271-278).  Names and
// handles live here on the host; each file's span table lives in HBM and all
// per-span work runs in files.hip.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/chunkfs_amd.h"
#include "../../include/chunkfs_amd_debug.h"
#include "delta.hpp"
#include "delta_plan.hpp"
#include "engine.hpp"
#include "files.hpp"
#include "diff_plan.hpp"
#include "pack.hpp"
#include "pack_plan.hpp"
#include "read_plan.hpp"
#include "splice_plan.hpp"
#include "store.hpp"
#include "store_internal.hpp"

namespace {

using cdc::DeviceBuf;
using cdc::PinnedBuf;
using word = unsigned long long;

struct FileRec {
    uint64_t n = 0;      // spans
    uint64_t size = 0;   // bytes = off[n]
    uint64_t cap = 0;    // spans the table holds
    uint64_t epoch = 0;  // the store's epoch when the spans were resolved
    uint64_t min_len = ~0ull;  // shortest span of length > 0 (~0: none yet)
    uint64_t zeros = 0;        // spans of length 0
    cdc::SpanTable t{};
};

// Span tables are carved out of larger device blocks, so that a new file costs
// no device allocation.  Capacities double from 64 spans: class c holds 64 << c.
// A table is one run of bytes, digest first (16-byte aligned for the uint4
// stores), then off, loc (8) and slot (4).  A block serves one class; freed
// tables go back to their class's list and the blocks are released with the layer.
constexpr uint64_t kTableMinCap = 64;
constexpr uint64_t kTableBlockBytes = 1ull << 20;

struct TablePool {
    std::vector<void *> blocks;
    std::vector<std::vector<uint8_t *>> free_tables;  // per class

    static uint64_t table_bytes(uint64_t cap) { return (cap * 52 + 8 + 255) & ~255ull; }
    static size_t class_of(uint64_t cap) { return (size_t)__builtin_ctzll(cap / kTableMinCap); }
    static cdc::SpanTable at(uint8_t *base, uint64_t cap) {
        cdc::SpanTable t{};
        t.digest = base;
        t.off = reinterpret_cast<uint64_t *>(base + cap * 32);
        t.loc = t.off + cap + 1;
        t.slot = reinterpret_cast<uint32_t *>(t.loc + cap);
        return t;
    }

    // cap: 64 << c.  A table larger than the block size gets a block of its own.
    hipError_t take(uint64_t cap, cdc::SpanTable *out) {
        const size_t c = class_of(cap);
        if (free_tables.size() <= c) free_tables.resize(c + 1);
        if (free_tables[c].empty()) {
            const uint64_t tb = table_bytes(cap), per = tb < kTableBlockBytes ? kTableBlockBytes / tb : 1;
            void *p = nullptr;
            const hipError_t e = hipMalloc(&p, per * tb);
            if (e != hipSuccess) return e;
            blocks.push_back(p);
            for (uint64_t i = per; i-- > 0;) free_tables[c].push_back(static_cast<uint8_t *>(p) + i * tb);
        }
        *out = at(free_tables[c].back(), cap);
        free_tables[c].pop_back();
        return hipSuccess;
    }
    void give(const cdc::SpanTable &t, uint64_t cap) {
        if (cap) free_tables[class_of(cap)].push_back(t.digest);
    }
    void release() {
        for (void *p : blocks) (void)hipFree(p);
        blocks.clear();
        free_tables.clear();
    }
};

// What the kernels hand back, one member per meaning.  A kernel that writes
// several words gets the address of the first: the members of one line are
// adjacent, in the order the comment at its launch_ function lists them.
struct HostWords {               // pinned host memory
    word appended;               // append, splice build, ratio gather: bytes appended (the derived file's size)
    word distinct;               // distribution: distinct slots
    word least, zeros;           // DeviceWords' copy
    word unique, unique_length;  // launch_files_ratio_unique: U and the bytes of the unique spans
    word cycle, partial;         // launch_files_ratio_take: C = bytes of one cycle, spans of the partial cycle
    word verify;                 // DeviceWords' copy
    word x_pieces, x_touched;    // launch_files_plan_x: pieces in all, target-kind spans touched
    word i0, w0;                 // launch_splice_start: the start span and off[i0]
    word resync_k, resync_j, resync_e;  // launch_splice_resync: the smallest chunk that resyncs (~0: none), the old
                                        // span its cut meets, the cut
    word ranges, bytes_differing, bytes_compared, bytes_shared, pieces;  // launch_files_diff
    word pack_chunks, pack_data;      // launch_pack_mark: carried chunks, bytes of the data section
    word pack_external, pack_bytes;   // DeviceWords' copy
    word delta[6];  // launch_files_delta: ops, bytes_copy, bytes_literal, bytes_literal_tables, spans_matched, regions
};
struct DeviceWords {
    word least, zeros;  // launch_files_append's d_stat, preset to {~0, 0}: min(length - 1) over the spans of
                        // length > 0, spans of length 0
    word verify;        // the smallest destination address - cmp_base at which a byte differs, preset to ~0
    word touch;         // launch_files_plan_x's counter
    word best;          // launch_splice_resync's
    word pack_external, pack_bytes;  // launch_pack_mark's d_acc: spans whose slot is excluded, unpadded bytes of
                                     // the carried chunks
};

// Scratch kept between calls, one struct per group of buffers that grow
// together (grow_group, store_internal.hpp); the rule is the group's own.
struct SpanScratch {  // append / distribution / ratio: per span
    uint64_t cap = 0;
    DeviceBuf<uint64_t> val, block;
    hipError_t grow(uint64_t n) {
        const uint64_t c = n + n / 8 + 64;
        return cdc::grow_group(cap, n, c, val, c, block, cdc::store_scan_blocks(c) + 1);
    }
};
struct SlotScratch {  // distribution / ratio: per slot, as large as the store's table
    uint64_t cap = 0;
    DeviceBuf<uint32_t> cnt;
    DeviceBuf<uint64_t> first;
    hipError_t grow(uint64_t slots) { return cdc::grow_group(cap, slots, slots, cnt, slots, first, slots); }
};
struct WriteScratch {  // write / batch write / splice: chunk list and digests of one call, n the chunker's bound
    uint64_t cap = 0;
    DeviceBuf<cdc_chunk_t> chunks;
    DeviceBuf<uint8_t> dig;
    hipError_t grow(uint64_t n) { return cdc::grow_group(cap, n, n, chunks, n, dig, n * 32); }
};
// What cdc_files_write_batch_device uploads in one copy, for n requests:
// first[n + 1], the destinations and the preset statistics.
uint64_t batch_bytes(uint64_t n) { return (n + 1) * 8 + n * (sizeof(cdc::AppendDst) + sizeof(cdc::AppendStat)); }
struct BatchUpload {
    uint64_t cap = 0;
    PinnedBuf<uint8_t> h;
    DeviceBuf<uint8_t> d;
    hipError_t grow(uint64_t n) {
        const uint64_t c = n + n / 8 + 16;
        return cdc::grow_group(cap, n, c, h, batch_bytes(c), d, batch_bytes(c));
    }
};
struct RequestScratch {  // reads: per request
    uint64_t cap = 0;
    PinnedBuf<cdc::ReadReq> h_req;
    PinnedBuf<cdc::ReadResult> h_res;
    DeviceBuf<cdc::ReadReq> d_req;
    DeviceBuf<cdc::ReadPlan> plan;
    DeviceBuf<uint64_t> cnt, block;
    hipError_t grow(uint64_t n) {
        const uint64_t c = n + n / 8 + 16;
        return cdc::grow_group(cap, n, c, h_req, c, h_res, c, d_req, c, plan, c, cnt, c, block,
                               cdc::store_scan_blocks(c) + 1);
    }
};
struct PackScratch {  // pack: per span, the rank and the padded offset of the carried chunks with their scans
    uint64_t cap = 0;
    DeviceBuf<uint64_t> rank, poff, bs_rank, bs_off;
    hipError_t grow(uint64_t n) {
        const uint64_t c = n + n / 8 + 64, b = cdc::store_scan_blocks(c) + 1;
        return cdc::grow_group(cap, n, c, rank, c, poff, c, bs_rank, b, bs_off, b);
    }
};
struct UnpackHost {  // unpack: what crosses to the host, pinned
    cdc::PackHeader header;
    cdc::PackResult res;
};
struct UnpackScratch {  // unpack: per span its slot; per carried chunk the hash that is compared with its digest
    uint64_t span_cap = 0, chunk_cap = 0;
    DeviceBuf<uint32_t> slot;
    DeviceBuf<uint8_t> sha;
    PinnedBuf<UnpackHost> h;
    DeviceBuf<cdc::PackResult> res;
    hipError_t grow(uint64_t spans, uint64_t chunks) {
        hipError_t e = h.room(1);
        if (e == hipSuccess) e = res.room(1);
        if (e == hipSuccess) e = cdc::grow_group(span_cap, spans, spans + spans / 8 + 64, slot, spans + spans / 8 + 64);
        if (e == hipSuccess)
            e = cdc::grow_group(chunk_cap, chunks, chunks + chunks / 8 + 64, sha, (chunks + chunks / 8 + 64) * 32);
        return e;
    }
};
struct SlotArrays {  // reads in the scrubbed state: per request, the address of its file's slot array
    uint64_t cap = 0;
    PinnedBuf<uint64_t> h;
    DeviceBuf<uint64_t> d;
    hipError_t grow(uint64_t n) {
        const uint64_t c = n + n / 8 + 16;
        return cdc::grow_group(cap, n, c, h, c, d, c);
    }
};

}  // namespace

struct cdc_files {
    cdc_store *store = nullptr;
    int device = 0;  // the store's, kept so that teardown needs nothing of the store
    uint64_t seg = 0;
    TablePool pool;
    std::map<std::string, FileRec *> files;  // ordered: cdc_files_list is deterministic
    std::set<cdc_fh *> handles;
    PinnedBuf<HostWords> hw;  // one each, allocated with the layer
    DeviceBuf<DeviceWords> dw;
    SpanScratch span;
    SlotScratch slot;
    WriteScratch wr;
    BatchUpload batch;
    RequestScratch req;
    cdc::ScanScratch<cdc::StorePiece> pc;  // reads: per piece, with the tile counts
    SlotArrays xslot;
    cdc::ScanScratch<cdc::SpanRec> xspan;  // reads in the scrubbed state: per span, with the piece counts
    DeviceBuf<uint8_t> window;  // cdc_file_splice_device: the window of the new file that is chunked
    DeviceBuf<uint8_t> diff;    // cdc_files_diff_device: one block carved into the DiffScratch arrays
    DeviceBuf<uint8_t> delta;   // cdc_files_delta_device: one block carved into the DeltaScratch arrays
    PackScratch pack;
    UnpackScratch unpack;
};

struct cdc_fh {
    cdc_files *fs = nullptr;  // NULL once the layer is destroyed
    std::string name;         // the reference's handle holds the name, not the file (file_layer.rs:32-41)
    bool readonly = false;
    uint64_t cursor = 0;      // FileHandle::offset as read_from_file uses it
    double chunk_s = 0, hash_s = 0;
};

namespace {

int code_of(hipError_t e) { return e == hipErrorOutOfMemory ? CDC_ENOMEM : CDC_EDEVICE; }

#define FL_TRY(expr)                                                         \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            cdc::set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
            return code_of(e_);                                              \
        }                                                                    \
    } while (0)

int fail(int code, const std::string &msg) {
    cdc::set_error(msg);
    return code;
}

int fail_hip(const std::string &what, hipError_t e) { return fail(code_of(e), what + hipGetErrorString(e)); }

// The table goes back to the layer's pool.  Every call synchronises its stream
// before it returns, so a table handed out again is no longer read or written.
void free_table(cdc_files *fs, FileRec *f) {
    fs->pool.give(f->t, f->cap);
    f->t = cdc::SpanTable{};
    f->cap = 0;
}

void drop_files(cdc_files *fs) {
    for (auto &kv : fs->files) {
        free_table(fs, kv.second);
        delete kv.second;
    }
    fs->files.clear();
}

// The capacity of a table that holds `cap` spans now and is to hold `need`.
uint64_t table_cap(uint64_t cap, uint64_t need) {
    if (!cap) cap = kTableMinCap;
    while (cap < need) cap *= 2;
    return cap;
}

// A table of that capacity from the pool; `what` opens the message when there is none.
int take_table(cdc_files *fs, uint64_t cap, cdc::SpanTable *t, const char *what) {
    const hipError_t e = fs->pool.take(cap, t);
    return e == hipSuccess ? CDC_OK : fail_hip(what, e);
}

// Queues the copy of n spans, and the offset that closes them.
hipError_t copy_spans(const cdc::SpanTable &to, const cdc::SpanTable &from, uint64_t n, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(to.off, from.off, (n + 1) * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(to.digest, from.digest, n * 32, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(to.loc, from.loc, n * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(to.slot, from.slot, n * 4, hipMemcpyDeviceToDevice, s);
    return e;
}

// Capacity doubles: a table of the next class from the pool, the spans copied on
// the call's stream, the old table back to the pool.  copied == NULL: the copy is
// waited for here.  Otherwise *copied is set when a copy was queued and the
// caller waits once for all of them; until then only work on `s` may follow.
int reserve(cdc_files *fs, FileRec *f, uint64_t need, hipStream_t s, bool *copied = nullptr) {
    if (need <= f->cap) return CDC_OK;
    const uint64_t cap = table_cap(f->cap, need);
    cdc::SpanTable t{};
    const int rc = take_table(fs, cap, &t, "file layer: span table growth: ");
    if (rc) return rc;
    if (f->n) {
        hipError_t e = copy_spans(t, f->t, f->n, s);
        if (e == hipSuccess && !copied) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(s);  // whatever was queued is done before the table is handed out again
            fs->pool.give(t, cap);
            return fail_hip("file layer: span table growth: ", e);
        }
        if (copied) *copied = true;
    }
    free_table(fs, f);
    f->t = t;
    f->cap = cap;
    return CDC_OK;
}

void release(cdc_files *fs) {
    (void)hipSetDevice(fs->device);
    drop_files(fs);
    for (cdc_fh *h : fs->handles) h->fs = nullptr;
    fs->pool.release();
    delete fs;  // the buffers free themselves, the device still current
}

// A file whose spans were resolved before the store was last cleared names
// slots of another table: nothing can be read from it or added to it.
int check_epoch(const cdc_files *fs, const FileRec *f, const std::string &name) {
    if (f->n && f->epoch != cdc::store_view(fs->store).epoch)
        return fail(CDC_ENOTFOUND, "file layer: the store was cleared since '" + name + "' was written");
    return CDC_OK;
}

// The handle's file, by name as the reference finds it (file_layer.rs:116-124).
// for_read: the spans must have been resolved under the store's current epoch.
int lookup(cdc_fh *fh, bool for_read, FileRec **out) {
    if (!fh) return fail(CDC_EINVAL, "NULL file handle");
    if (!fh->fs) return fail(CDC_EINVAL, "file handle outlived its file layer");
    auto it = fh->fs->files.find(fh->name);
    if (it == fh->fs->files.end()) return fail(CDC_ENOTFOUND, "file layer: no file named '" + fh->name + "'");
    *out = it->second;
    return for_read ? check_epoch(fh->fs, it->second, fh->name) : CDC_OK;
}

// The handle's file for a call that adds spans to it.
int writable(cdc_fh *fh, FileRec **out) {
    const int rc = lookup(fh, false, out);
    if (rc) return rc;
    if (fh->readonly) return fail(CDC_EPERM, "file handle is read-only");
    return check_epoch(fh->fs, *out, fh->name);
}

hipStream_t stream_of(cdc_files *fs, void *hip_stream) {
    return hip_stream ? static_cast<hipStream_t>(hip_stream) : cdc::store_view(fs->store).stream;
}

// Around a launch that takes d_stat: the preset, the copy to the host, and what
// the host keeps of it per file to bound the spans of a range (read_plan.hpp).
hipError_t preset_stat(cdc_files *fs, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(&fs->dw->least, 0xFF, sizeof(word), s);
    return e == hipSuccess ? hipMemsetAsync(&fs->dw->zeros, 0, sizeof(word), s) : e;
}
hipError_t fetch_stat(cdc_files *fs, hipStream_t s) {
    return hipMemcpyAsync(&fs->hw->least, &fs->dw->least, 2 * sizeof(word), hipMemcpyDeviceToHost, s);
}
void fold_stat(FileRec *f, uint64_t least, uint64_t zeros) {
    if (least != ~0ull && least + 1 < f->min_len) f->min_len = least + 1;
    f->zeros += zeros;
}

int64_t append(cdc_fh *fh, const uint8_t *d_data, uint64_t data_len, const cdc_chunk_t *d_chunks,
               const uint8_t *d_digests, uint64_t n, void *hip_stream) {
    FileRec *f = nullptr;
    int rc = writable(fh, &f);
    if (rc) return rc;
    cdc_files *fs = fh->fs;
    cdc::StoreView v = cdc::store_view(fs->store);
    if (n == 0) return 0;
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    if ((rc = reserve(fs, f, f->n + n, s)) != CDC_OK) return rc;
    FL_TRY(fs->span.grow(n));
    const int64_t put = cdc::store_put_slots(fs->store, d_data, data_len, d_chunks, d_digests, n, hip_stream);
    if (put < 0) return put;  // refused: the file is as it was
    v = cdc::store_view(fs->store);
    FL_TRY(preset_stat(fs, s));
    FL_TRY(cdc::launch_files_append(f->t, f->n, f->size, v.slot_of, v.length, v.loc, d_digests, n, fs->span.val,
                                    fs->span.block, &fs->dw->least, &fs->hw->appended, s));
    FL_TRY(fetch_stat(fs, s));
    FL_TRY(hipStreamSynchronize(s));
    f->n += n;
    f->size += fs->hw->appended;
    f->epoch = v.epoch;
    fold_stat(f, fs->hw->least, fs->hw->zeros);
    return (int64_t)n;
}

// One request of `kind` on a file; cap, the destination's size, also bounds the tiles.
struct HostReq {
    FileRec *f;
    uint32_t kind;
    uint64_t a, b;
    uint8_t *dst;
    uint64_t cap;
    cdc_chunk_t *spans;
};

// The host-side bounds of a call, summed over its requests (read_plan.hpp):
// spans touched, bytes copied, and the tiles of the requests that have bytes.
struct ReadTotals {
    uint64_t spans = 0, bytes = 0, tiles = 0;
};
// Room for the requests, fs->req.h_req filled, the bounds summed.
int prepare_reads(cdc_files *fs, const std::vector<HostReq> &reqs, ReadTotals *t) {
    FL_TRY(fs->req.grow(reqs.size()));
    for (uint64_t i = 0; i < reqs.size(); ++i) {
        const HostReq &q = reqs[i];
        fs->req.h_req[i] = cdc::ReadReq{q.f->t.off, q.f->t.loc, q.f->n, q.a, q.b, (uint64_t)(uintptr_t)q.dst, q.cap,
                                        (uint64_t)(uintptr_t)q.spans, q.kind, 0};
        const cdc::ReadBound b = cdc::read_bound(q.kind, q.b, q.cap, q.f->n, q.f->size, q.f->min_len, q.f->zeros);
        t->spans += b.spans;
        t->bytes += b.bytes;
        if (b.bytes) t->tiles += cdc::read_tiles_bound(b.bytes, b.spans);
    }
    return CDC_OK;
}

// run_reads once the store holds target-kind containers: a span's bytes are
// found through its slot's current container, and a span yields one piece per
// key.  The exact piece count is read back before the copy (one more host wait
// than the unscrubbed path): a sub-chunk may be one byte long, so a bound from
// the byte count alone would be the byte count.
int run_reads_scrubbed(cdc_files *fs, const std::vector<HostReq> &reqs, const cdc::ScrubView &sv, bool stale,
                       void *hip_stream, const uint8_t *cmp_base) {
    const cdc::StoreView v = cdc::store_view(fs->store);
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    const uint64_t nreq = reqs.size();
    ReadTotals max;  // span lengths only: as unscrubbed
    int rc = prepare_reads(fs, reqs, &max);
    if (rc) return rc;
    FL_TRY(fs->xslot.grow(nreq));
    FL_TRY(fs->xspan.grow(max.spans));
    cdc::ReadReq *h_req = fs->req.h_req;
    for (uint64_t i = 0; i < nreq; ++i) fs->xslot.h[i] = (uint64_t)(uintptr_t)reqs[i].f->t.slot;
    if (stale)  // nothing may be written if the read turns out to need the cleared target: spans go out after the check
        for (uint64_t i = 0; i < nreq; ++i) h_req[i].spans = 0;
    auto plan = [&] {
        return cdc::launch_files_plan_x(fs->req.d_req, fs->xslot.d, nreq, sv, fs->req.plan, fs->req.cnt, fs->req.block,
                                        fs->xspan.items, fs->xspan.val, fs->xspan.block, max.spans, fs->req.h_res,
                                        &fs->dw->touch, &fs->hw->x_pieces, s);
    };
    FL_TRY(hipMemcpyAsync(fs->req.d_req, h_req, nreq * sizeof(cdc::ReadReq), hipMemcpyHostToDevice, s));
    FL_TRY(hipMemcpyAsync(fs->xslot.d, fs->xslot.h, nreq * 8, hipMemcpyHostToDevice, s));
    FL_TRY(plan());
    FL_TRY(hipStreamSynchronize(s));
    if (stale && fs->hw->x_touched)
        return fail(CDC_ENOTFOUND, "file layer: the target store was cleared since these chunks were scrubbed");
    if (stale) {  // every span touched is chunk-kind: plan again, with the span output
        bool any = false;
        for (uint64_t i = 0; i < nreq; ++i) any = any || reqs[i].spans;
        if (any) {
            for (uint64_t i = 0; i < nreq; ++i) h_req[i].spans = (uint64_t)(uintptr_t)reqs[i].spans;
            FL_TRY(hipMemcpyAsync(fs->req.d_req, h_req, nreq * sizeof(cdc::ReadReq), hipMemcpyHostToDevice, s));
            FL_TRY(plan());
            FL_TRY(hipStreamSynchronize(s));
        }
    }
    const uint64_t np = fs->hw->x_pieces;
    if (!np) return CDC_OK;
    FL_TRY(fs->pc.grow(np));
    FL_TRY(cdc::launch_files_copy_x(fs->xspan.items, fs->xspan.val, max.spans, sv, v.loc, (uint64_t)(uintptr_t)v.arena,
                                    fs->pc.items, fs->pc.val, fs->pc.block, np,
                                    cdc::read_tiles_bound(max.bytes, np), s, (uint64_t)(uintptr_t)cmp_base,
                                    cmp_base ? &fs->dw->verify : nullptr));
    if (cmp_base) FL_TRY(hipMemcpyAsync(&fs->hw->verify, &fs->dw->verify, sizeof(word), hipMemcpyDeviceToHost, s));
    FL_TRY(hipStreamSynchronize(s));
    return CDC_OK;
}

// Plans and copies every request in one pass; fs->req.h_res[i] holds the
// results.  cmp_base (verify): the destinations are compared with the file's
// bytes instead of written; fs->hw->verify = the smallest destination address
// - cmp_base at which a byte differs, ~0 when none does.
int run_reads(cdc_files *fs, const std::vector<HostReq> &reqs, void *hip_stream, const uint8_t *cmp_base = nullptr) {
    if (cmp_base) {
        FL_TRY(hipSetDevice(cdc::store_view(fs->store).device));
        fs->hw->verify = ~0ull;
        FL_TRY(hipMemsetAsync(&fs->dw->verify, 0xFF, sizeof(word), stream_of(fs, hip_stream)));
    }
    {
        cdc::ScrubView sv;
        bool stale = false;
        if (cdc::store_scrub_view(fs->store, &sv, &stale))
            return run_reads_scrubbed(fs, reqs, sv, stale, hip_stream, cmp_base);
    }
    const cdc::StoreView v = cdc::store_view(fs->store);
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    const uint64_t nreq = reqs.size();
    ReadTotals max;
    const int rc = prepare_reads(fs, reqs, &max);
    if (rc) return rc;
    FL_TRY(fs->pc.grow(max.spans));
    FL_TRY(hipMemcpyAsync(fs->req.d_req, fs->req.h_req, nreq * sizeof(cdc::ReadReq), hipMemcpyHostToDevice, s));
    FL_TRY(cdc::launch_files_read(fs->req.d_req, nreq, (uint64_t)(uintptr_t)v.arena, fs->req.plan, fs->req.cnt,
                                  fs->req.block, fs->pc.items, fs->pc.val, fs->pc.block, max.spans, max.tiles,
                                  fs->req.h_res, s, (uint64_t)(uintptr_t)cmp_base,
                                  cmp_base ? &fs->dw->verify : nullptr));
    if (cmp_base) FL_TRY(hipMemcpyAsync(&fs->hw->verify, &fs->dw->verify, sizeof(word), hipMemcpyDeviceToHost, s));
    FL_TRY(hipStreamSynchronize(s));
    return CDC_OK;
}

int64_t read_one(cdc_fh *fh, uint32_t kind, uint64_t a, uint64_t b, uint8_t *d_out, uint64_t cap,
                 cdc_chunk_t *d_spans, void *hip_stream) {
    FileRec *f = nullptr;
    int rc = lookup(fh, true, &f);
    if (rc) return rc;
    if (cap && !d_out) return fail(CDC_EINVAL, "file layer read: NULL destination");
    if (f->n == 0) return 0;
    std::vector<HostReq> reqs{HostReq{f, kind, a, b, d_out, cap, d_spans}};
    if ((rc = run_reads(fh->fs, reqs, hip_stream)) != CDC_OK) return rc;
    return (int64_t)fh->fs->req.h_res[0].bytes;
}

// ---- splice ---------------------------------------------------------------------
double *splice_split() {
    static thread_local double split[5];
    return split;
}

int64_t splice(cdc_fh *fh, cdc_handle_t *chunker, uint64_t offset, uint64_t remove_len, const uint8_t *d_data,
               uint64_t insert_len, cdc_splice_stats_t *out, void *hip_stream) {
    // Everything that can refuse, before any device work.
    if (!fh) return fail(CDC_EINVAL, "cdc_file_splice_device: NULL file handle");
    if (!chunker) return fail(CDC_EINVAL, "cdc_file_splice_device: NULL chunker");
    if (insert_len && !d_data) return fail(CDC_EINVAL, "cdc_file_splice_device: NULL data");
    FileRec *f = nullptr;
    int rc = writable(fh, &f);
    if (rc) return rc;
    cdc_files *fs = fh->fs;
    cdc::StoreView v = cdc::store_view(fs->store);
    const uint64_t n = f->n, size = f->size;
    if (offset > size)
        return fail(CDC_EINVAL, "cdc_file_splice_device: offset " + std::to_string(offset) + " is past the file's " +
                                    std::to_string(size) + " bytes");
    if (!cdc::splice_range_ok(size, offset, remove_len))
        return fail(CDC_EINVAL, "cdc_file_splice_device: offset + remove_len is past the file's " +
                                    std::to_string(size) + " bytes");
    uint64_t size_after = 0;
    if (!cdc::splice_size_after(size, remove_len, insert_len, &size_after))
        return fail(CDC_EINVAL, "cdc_file_splice_device: insert_len makes the file larger than 2^64 bytes");
    if (cdc::handle_device(chunker) != v.device)
        return fail(CDC_EINVAL, "cdc_file_splice_device: the chunker is on another device than the store");
    {
        cdc::ScrubView sv;
        bool stale = false;
        if (cdc::store_scrub_view(fs->store, &sv, &stale))
            return fail(CDC_ENOTSUP, "cdc_file_splice_device: the store holds target-kind containers (scrubbed); "
                                     "not supported");
    }
    if (!remove_len && !insert_len) return 0;

    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    double split[5] = {0, 0, 0, 0, 0};
    auto last = std::chrono::steady_clock::now();
    auto lap = [&](int phase) {
        const auto now = std::chrono::steady_clock::now();
        split[phase] += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    };

    // 1. The start span.
    uint64_t i0 = 0, w0 = 0;
    if (n) {
        FL_TRY(cdc::launch_splice_start(f->t.off, n, offset, &fs->hw->i0, s));
        FL_TRY(hipStreamSynchronize(s));
        i0 = fs->hw->i0;
        w0 = fs->hw->w0;
    }

    // 2, 3. Windows of the new file from off[i0] on, until a trusted cut meets an old one.
    const uint64_t maxc = cdc::handle_max_chunk(chunker), lo = offset + insert_len;
    uint64_t j = n, e = size_after, m = 0, wlen = 0, window_bytes = 0;
    uint32_t rounds = 1;
    const uint8_t *streams[1] = {nullptr};
    for (uint32_t round = 1; size_after > w0; ++round) {
        const uint64_t end_w = cdc::splice_window_end(size_after, offset, insert_len, maxc, round);
        wlen = end_w - w0;
        if (fs->window.cap < wlen) FL_TRY(fs->window.room((wlen + wlen / 8 + 4095) & ~4095ull));
        uint8_t *win = fs->window;
        streams[0] = win;
        std::vector<HostReq> reqs;
        if (offset > w0) reqs.push_back(HostReq{f, cdc::kReadRange, w0, offset - w0, win, offset - w0, nullptr});
        if (end_w > lo)
            reqs.push_back(HostReq{f, cdc::kReadRange, offset + remove_len, end_w - lo, win + (lo - w0), end_w - lo,
                                   nullptr});
        if (!reqs.empty() && (rc = run_reads(fs, reqs, hip_stream)) != CDC_OK) return rc;
        if (insert_len)
            FL_TRY(hipMemcpyAsync(win + (offset - w0), d_data, insert_len, hipMemcpyDeviceToDevice, s));
        lap(0);
        const uint64_t lens[1] = {wlen};
        const uint64_t cap = cdc_batch_max_chunks(chunker, 1, lens);
        FL_TRY(fs->wr.grow(cap));
        uint64_t first[2] = {0, 0};
        const int64_t cnt = cdc_chunk_batch_device(chunker, 1, streams, lens, fs->wr.chunks, cap, first, s);
        if (cnt < 0) return cnt;
        window_bytes += wlen;
        rounds = round;
        lap(1);
        const cdc::SpliceRound r{w0, end_w, size_after, offset, remove_len, insert_len, maxc};
        FL_TRY(cdc::launch_splice_resync(reinterpret_cast<const cdc::cdc_chunk_pod *>(fs->wr.chunks.p), (uint64_t)cnt,
                                         r, f->t.off, n, &fs->dw->best, &fs->hw->resync_k, s));
        FL_TRY(hipStreamSynchronize(s));
        lap(2);
        if (fs->hw->resync_k != ~0ull) {
            m = fs->hw->resync_k + 1;
            j = fs->hw->resync_j;
            e = fs->hw->resync_e;
            break;
        }
        if (end_w == size_after)  // the last cut of a window that ends with the file is the file's end
            return fail(CDC_EDEVICE, "cdc_file_splice_device: the chunks do not end where the file does");
    }

    // 4. Hash and put the accepted chunks, then the table.
    const uint64_t n_new = i0 + m + (n - j);
    uint64_t bytes_new = 0;
    if (m) {
        const uint64_t hfirst[2] = {0, m};
        if ((rc = cdc_hash_batch_device(chunker, cdc_store_hash(fs->store), 1, streams, hfirst, fs->wr.chunks, fs->wr.dig, s)) != CDC_OK) return rc;
        const bool patch = m == j - i0 && insert_len == remove_len;
        cdc::SpanTable nt = f->t;
        uint64_t cap = f->cap;
        if (!patch) {
            cap = table_cap(cap, n_new);
            if ((rc = take_table(fs, cap, &nt, "file layer: span table for the splice: ")) != CDC_OK) return rc;
        }
        struct Guard {  // the fresh table goes back unless the call succeeds
            cdc_files *fs;
            cdc::SpanTable t;
            uint64_t cap;
            ~Guard() {
                if (cap) fs->pool.give(t, cap);
            }
        } guard{fs, nt, patch ? 0 : cap};
        FL_TRY(fs->span.grow(m));
        cdc_store_stats_t before{}, after{};
        (void)cdc_store_stats(fs->store, &before);
        const int64_t put = cdc::store_put_slots(fs->store, fs->window, wlen, fs->wr.chunks, fs->wr.dig, m, hip_stream);
        if (put < 0) return put;  // refused: the file and its table are as they were
        (void)cdc_store_stats(fs->store, &after);
        bytes_new = after.index.unique_bytes - before.index.unique_bytes;
        v = cdc::store_view(fs->store);
        lap(3);
        hipError_t he = preset_stat(fs, s);
        if (he == hipSuccess)
            he = cdc::launch_splice_build(f->t, n, size, nt, i0, j, w0, remove_len, insert_len, v.slot_of, v.length,
                                          v.loc, fs->wr.dig, m, fs->span.val, fs->span.block, &fs->dw->least,
                                          &fs->hw->appended, s);
        if (he == hipSuccess) he = fetch_stat(fs, s);
        const hipError_t hs = hipStreamSynchronize(s);  // also on failure: nothing queued still writes the fresh table
        if (he == hipSuccess) he = hs;
        if (he != hipSuccess) {
            cdc::set_error(std::string("cdc_file_splice_device: table build: ") + hipGetErrorString(he));
            return CDC_EDEVICE;
        }
        if (!patch) {
            free_table(fs, f);
            f->t = nt;
            f->cap = cap;
            guard.cap = 0;
        }
        fold_stat(f, fs->hw->least, fs->hw->zeros);
        lap(4);
    } else {
        free_table(fs, f);  // nothing is left after off[i0] = 0: the file is empty
    }
    f->n = n_new;
    f->size = size_after;
    f->epoch = v.epoch;
    std::memcpy(splice_split(), split, sizeof split);
    if (out)
        *out = cdc_splice_stats_t{i0, j - i0, m, e, size, size_after, bytes_new, window_bytes, rounds, 0};
    return (int64_t)m;
}

// ---- diff -----------------------------------------------------------------------
// The diff's scratch for two tables of na and nb spans: every size is a bound
// the host has before the first launch.  A piece starts at a span boundary, so
// there are at most na + nb of them; a compared piece adds at most two ragged
// tiles to its whole ones.  The mask is 64 words per tile: one bit per compared
// byte plus, per piece, the two tiles' worth that its ends may leave unused.
int grow_diff(cdc_files *fs, uint64_t na, uint64_t nb, uint64_t common, bool tables_only, cdc::DiffScratch *w) {
    const uint64_t nc = cdc::diff_candidates(na, nb), mp = na + nb;
    const uint64_t mt = tables_only ? 0 : common / cdc::kStoreTile + 2 * mp;
    const uint64_t words = 4 /* acc */ + nc + 4 * mp /* pstart, pflag, tstart, cx */ + 3 * mp /* cp */ +
                           mt * (1 + cdc::kDiffTileWords) + cdc::store_scan_blocks(nc) + 1 +
                           2 * (cdc::store_scan_blocks(mp) + 1) + cdc::store_scan_blocks(mt) + 1;
    const uint64_t bytes = words * 8 + 3 * mp * 4 /* pia, pib, cflag */;
    if (fs->diff.cap < bytes) FL_TRY(fs->diff.room(bytes + bytes / 8));
    uint64_t *p = reinterpret_cast<uint64_t *>(fs->diff.p);
    auto take = [&p](uint64_t n) {
        uint64_t *r = p;
        p += n;
        return r;
    };
    static_assert(sizeof(cdc::StorePiece) == 24, "three words");
    w->acc = reinterpret_cast<unsigned long long *>(take(4));
    w->cand = take(nc);
    w->pstart = take(mp);
    w->pflag = take(mp);
    w->tstart = take(mp);
    w->cx = take(mp);
    w->cp = reinterpret_cast<cdc::StorePiece *>(take(3 * mp));
    w->tcount = take(mt);
    w->mask = take(mt * cdc::kDiffTileWords);
    w->bs_c = take(cdc::store_scan_blocks(nc) + 1);
    w->bs_p = take(cdc::store_scan_blocks(mp) + 1);
    w->bs_t = take(cdc::store_scan_blocks(mp) + 1);
    w->bs_r = take(cdc::store_scan_blocks(mt) + 1);
    w->n_pieces = w->bs_c + cdc::store_scan_blocks(nc);
    w->n_cmp = w->bs_p + cdc::store_scan_blocks(mp);
    w->n_tiles = w->bs_t + cdc::store_scan_blocks(mp);
    w->n_starts = w->bs_r + cdc::store_scan_blocks(mt);
    uint32_t *q = reinterpret_cast<uint32_t *>(p);
    w->pia = q;
    w->pib = q + mp;
    w->cflag = q + 2 * mp;
    w->max_pieces = mp;
    w->max_tiles = mt;
    return CDC_OK;
}

// ---- delta ----------------------------------------------------------------------
// The delta's scratch for two tables of na and nb > 0 spans, one block as the
// diff's is.  A run begins at a span of B, so there are at most nb of them; a
// region adds at most one ragged tile to its whole ones; a region opens at most
// three ops and a COPY run one, and regions alternate with COPY runs.
int grow_delta(cdc_files *fs, uint64_t na, uint64_t nb, uint64_t size_b, hipStream_t s, cdc::DeltaScratch *w) {
    const uint64_t sb = cdc::store_scan_blocks(nb) + 1;
    size_t sort_bytes = 0;
    FL_TRY(cdc::launch_retain_sort(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, na, 32, s));
    const uint64_t words = 4 /* acc */ + 2 * na /* key_in, key */ + nb /* diag */ + nb /* rflag */ +
                           2 * (nb + 1) /* rb, rd */ + 4 * nb /* tstart, fwd, bwd, hcount */ + 6 * nb /* hb, ha */ +
                           3 * sb;
    const uint64_t idx_at = words * 8, sort_at = (idx_at + 2 * na * 4 + 255) & ~255ull;
    const uint64_t bytes = sort_at + sort_bytes;
    if (fs->delta.cap < bytes) FL_TRY(fs->delta.room(bytes + bytes / 8));
    uint64_t *p = reinterpret_cast<uint64_t *>(fs->delta.p);
    auto take = [&p](uint64_t n) {
        uint64_t *r = p;
        p += n;
        return r;
    };
    w->acc = reinterpret_cast<unsigned long long *>(take(4));
    w->key_in = take(na);
    w->key = take(na);
    w->diag = reinterpret_cast<int64_t *>(take(nb));
    w->rflag = take(nb);
    w->rb = take(nb + 1);
    w->rd = reinterpret_cast<int64_t *>(take(nb + 1));
    w->tstart = take(nb);
    w->fwd = reinterpret_cast<unsigned long long *>(take(nb));
    w->bwd = reinterpret_cast<unsigned long long *>(take(nb));
    w->hcount = take(nb);
    w->hb = take(3 * nb);
    w->ha = take(3 * nb);
    w->bs_r = take(sb);
    w->bs_t = take(sb);
    w->bs_h = take(sb);
    w->n_runs = w->bs_r + sb - 1;
    w->n_tiles = w->bs_t + sb - 1;
    w->n_ops = w->bs_h + sb - 1;
    w->idx_in = reinterpret_cast<uint32_t *>(fs->delta.p + idx_at);
    w->idx = w->idx_in + na;
    w->sort_tmp = fs->delta.p + sort_at;
    w->sort_bytes = sort_bytes;
    w->max_tiles = size_b / cdc::kDeltaTile + nb;
    return CDC_OK;
}

// ---- packs ------------------------------------------------------------------------
bool scrubbed(const cdc_files *fs) {
    cdc::ScrubView sv;
    bool stale = false;
    return cdc::store_scrub_view(fs->store, &sv, &stale);
}

int pack_check_failed(uint32_t check, uint64_t index, uint64_t count) {
    return fail(CDC_EINVAL, std::string("cdc_files_unpack_device: pack check '") + cdc::pack_check_name(check) +
                                "' failed at index " + std::to_string(index) + " (" + std::to_string(count) +
                                " in all)");
}

// cdc_debug_pack_split: [0..1] the last pack of this thread, [2..6] the last unpack.
double *pack_split() {
    static thread_local double split[7];
    return split;
}
struct Laps {  // wall milliseconds between the call's host waits
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    double ms[5] = {0, 0, 0, 0, 0};
    void lap(int phase) {
        const auto now = std::chrono::steady_clock::now();
        ms[phase] += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    }
};

int64_t pack_file(cdc_fh *fh, cdc_fh *since, const uint8_t *d_have, uint8_t *d_pack, uint64_t cap,
                  cdc_pack_stats_t *stats, void *hip_stream) {
    const auto t0 = std::chrono::steady_clock::now();
    // Everything that can refuse, before any device work.
    if ((uintptr_t)d_pack & (cdc::kPackAlign - 1))
        return fail(CDC_EINVAL, "cdc_file_pack_device: d_pack is not 16-byte aligned");
    if (!fh) return fail(CDC_EINVAL, "cdc_file_pack_device: NULL file handle");
    if (cap && !d_pack) return fail(CDC_EINVAL, "cdc_file_pack_device: NULL destination");
    if (since && fh->fs && since->fs && since->fs != fh->fs)
        return fail(CDC_EINVAL, "cdc_file_pack_device: `since` belongs to another file layer");
    FileRec *f = nullptr, *base = nullptr;
    int rc = lookup(fh, true, &f);
    if (rc) return rc;
    if (since && (rc = lookup(since, true, &base)) != CDC_OK) return rc;
    cdc_files *fs = fh->fs;
    if (scrubbed(fs))
        return fail(CDC_ENOTSUP, "cdc_file_pack_device: the store holds target-kind containers (scrubbed); "
                                 "not supported");
    const cdc::StoreView v = cdc::store_view(fs->store);
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    const uint64_t n = f->n;
    Laps laps;

    // (a), (b): which chunks are carried and where; the one wait for the sizes.
    cdc::PackHeader h{cdc::kPackMagic, cdc::kPackVersion, cdc::pack_flags((uint32_t)cdc_store_hash(fs->store)), f->size, n, 0, 0, 0, 0};
    uint64_t chunk_bytes = 0;
    if (n) {
        FL_TRY(fs->pack.grow(n));
        FL_TRY(fs->slot.grow(v.slots));
        const uint64_t ns = base ? base->n : 0;
        FL_TRY(cdc::launch_pack_mark(f->t, n, ns ? base->t.slot : nullptr, ns, d_have, v.slots, fs->slot.cnt,
                                     fs->slot.first, fs->pack.rank, fs->pack.poff, fs->pack.bs_rank, fs->pack.bs_off,
                                     &fs->dw->pack_external, &fs->hw->pack_chunks, s));
        FL_TRY(hipMemcpyAsync(&fs->hw->pack_external, &fs->dw->pack_external, 2 * sizeof(word),
                              hipMemcpyDeviceToHost, s));
        FL_TRY(hipStreamSynchronize(s));
        h.n_chunks = fs->hw->pack_chunks;
        h.data_bytes = fs->hw->pack_data;
        h.external_spans = fs->hw->pack_external;
        chunk_bytes = fs->hw->pack_bytes;
    }
    laps.lap(0);
    cdc::PackLayout l{};
    if (!cdc::pack_layout(n, h.n_chunks, h.data_bytes, &l))
        return fail(CDC_EINVAL, "cdc_file_pack_device: the pack would be larger than 2^64 bytes");
    h.total_bytes = l.total;
    cdc_pack_stats_t r{};
    r.spans = n;
    r.chunks = h.n_chunks;
    r.external_spans = h.external_spans;
    r.chunk_bytes = chunk_bytes;
    r.pack_bytes = l.total;
    r.file_size = f->size;
    if (l.total <= cap) {
        // (c), (d): everything but the data in one kernel, the data through the store's copy.
        FL_TRY(fs->pc.grow(h.n_chunks));
        FL_TRY(cdc::launch_pack_write(f->t, n, fs->slot.cnt, fs->slot.first, fs->pack.rank, fs->pack.poff, h, l,
                                      d_pack, (uint64_t)(uintptr_t)v.arena, fs->pc.items, fs->pc.val, fs->pc.block,
                                      s));
        FL_TRY(hipStreamSynchronize(s));
    }
    laps.lap(1);
    std::memcpy(pack_split(), laps.ms, 2 * sizeof(double));
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = r;
    return (int64_t)l.total;
}

int64_t unpack_file(cdc_files *fs, const char *name, const uint8_t *d_pack, uint64_t len, cdc_handle_t *hasher,
                    uint32_t flags, cdc_pack_stats_t *stats, void *hip_stream) {
    const auto t0 = std::chrono::steady_clock::now();
    // 1. Arguments.
    if (flags & ~(uint32_t)CDC_UNPACK_TRUST)
        return fail(CDC_EINVAL, "cdc_files_unpack_device: unknown flag bits " + std::to_string(flags));
    if ((uintptr_t)d_pack & (cdc::kPackAlign - 1))
        return fail(CDC_EINVAL, "cdc_files_unpack_device: d_pack is not 16-byte aligned");
    if (len < cdc::kPackHeaderBytes)
        return fail(CDC_EINVAL, "cdc_files_unpack_device: " + std::to_string(len) + " bytes are no pack (len < 64)");
    if (!fs || !name || !d_pack) return fail(CDC_EINVAL, "cdc_files_unpack_device: NULL argument");
    const bool trust = (flags & CDC_UNPACK_TRUST) != 0;
    if (!hasher && !trust) return fail(CDC_EINVAL, "cdc_files_unpack_device: NULL hasher without CDC_UNPACK_TRUST");
    cdc::StoreView v = cdc::store_view(fs->store);
    if (hasher && cdc::handle_device(hasher) != v.device)
        return fail(CDC_EINVAL, "cdc_files_unpack_device: the hasher is on another device than the store");
    if (fs->files.count(name)) return fail(CDC_EEXIST, std::string("file layer: '") + name + "' already exists");
    if (scrubbed(fs))
        return fail(CDC_ENOTSUP, "cdc_files_unpack_device: the store holds target-kind containers (scrubbed); "
                                 "not supported");
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);

    Laps laps;

    // 2. Structure: the header on the host, the index sections in one kernel.
    FL_TRY(fs->unpack.grow(0, 0));
    UnpackHost *host = fs->unpack.h;
    FL_TRY(hipMemcpyAsync(&host->header, d_pack, sizeof host->header, hipMemcpyDeviceToHost, s));
    FL_TRY(hipStreamSynchronize(s));
    const cdc::PackHeader h = host->header;
    laps.lap(0);
    cdc::PackLayout l{};
    uint32_t bad = cdc::pack_check_header(h, len, &l, (uint32_t)cdc_store_hash(fs->store));
    if (!bad && h.n_spans >= 0xFFFFFFFFull) bad = cdc::kPackSizesCheck;  // a put's own limit
    if (bad) return pack_check_failed(bad, 0, 1);
    const uint64_t n = h.n_spans, nc = h.n_chunks;
    const cdc::PackView view = cdc::pack_view(d_pack, h, l);
    // Every allocation of the call: one that fails is a refusal.
    FL_TRY(fs->unpack.grow(n, nc));
    FL_TRY(fs->wr.grow(nc));
    FL_TRY(fs->span.grow(n));
    host = fs->unpack.h;
    cdc::PackResult *d_res = fs->unpack.res;
    FL_TRY(cdc::pack_result_preset(d_res, s));
    FL_TRY(cdc::launch_pack_validate(view, d_res, s));
    // 3. Externals: the lookup reads the digests, lengths and span_chunk at [0, n) only, so it may run
    // before the validation's verdict is known.
    FL_TRY(cdc::launch_pack_lookup(cdc::store_index(fs->store), view, fs->unpack.slot, d_res, s));
    FL_TRY(hipMemcpyAsync(&host->res, d_res, sizeof host->res, hipMemcpyDeviceToHost, s));
    FL_TRY(hipStreamSynchronize(s));
    {
        const cdc::PackResult &res = host->res;
        for (uint32_t c = cdc::kPackFirstDeviceCheck; c < cdc::kPackChecks; ++c)
            if (res.count[c]) return pack_check_failed(c, res.first[c], res.count[c]);
        if (!cdc::pack_ok_file_size(view, cdc::PackSum{res.sum_low, res.sum_wraps}))
            return pack_check_failed(cdc::kPackFileSizeCheck, n, 1);
        if (res.externals != h.external_spans) return pack_check_failed(cdc::kPackExternalCheck, res.externals, 1);
        if (res.missing)
            return fail(CDC_ENOTFOUND, "cdc_files_unpack_device: the store does not hold the chunk of external span " +
                                           std::to_string(res.missing_first) + " (" + std::to_string(res.missing) +
                                           " missing in all)");
        if (res.mislen)
            return fail(CDC_EINVAL, "cdc_files_unpack_device: the store holds the chunk of external span " +
                                        std::to_string(res.mislen_first) + " with another length than the pack states");
    }

    laps.lap(1);

    // 4. Integrity.
    const uint8_t *data = d_pack + l.data;
    if (nc) FL_TRY(cdc::launch_pack_gather(view, fs->wr.chunks, fs->wr.dig, s));
    if (nc && !trust) {
        const uint8_t *streams[1] = {data};
        const uint64_t first[2] = {0, nc};
        const int rc = cdc_hash_batch_device(hasher, cdc_store_hash(fs->store), 1, streams, first, fs->wr.chunks, fs->unpack.sha, s);
        if (rc) return rc;
        FL_TRY(cdc::launch_pack_verify(fs->unpack.sha, fs->wr.dig, nc, d_res, s));
        FL_TRY(hipMemcpyAsync(&host->res, d_res, sizeof host->res, hipMemcpyDeviceToHost, s));
        FL_TRY(hipStreamSynchronize(s));
        if (host->res.mismatch)
            return fail(CDC_EINVAL, "cdc_files_unpack_device: the data of carried chunk " +
                                        std::to_string(host->res.mismatch_first) + " does not hash to its digest (" +
                                        std::to_string(host->res.mismatch) + " in all)");
    }

    laps.lap(2);

    // 5. The put of the carried chunks; the table first, so that nothing can fail for memory after it.
    FileRec made;
    if (n) {
        const uint64_t cap = table_cap(0, n);
        const int rc = take_table(fs, cap, &made.t, "cdc_files_unpack_device: span table: ");
        if (rc) return rc;
        made.cap = cap;
    }
    struct Guard {  // the table goes back unless the call succeeds
        cdc_files *fs;
        FileRec *f;
        ~Guard() {
            if (f) free_table(fs, f);
        }
    } guard{fs, &made};
    cdc_store_stats_t before{}, after{};
    (void)cdc_store_stats(fs->store, &before);
    int64_t put = 0;
    if (nc) {
        put = cdc::store_put_slots(fs->store, data, h.data_bytes, fs->wr.chunks, fs->wr.dig, nc, s);
        if (put < 0) return put;  // refused: the store and the layer are as they were
    }
    (void)cdc_store_stats(fs->store, &after);
    const uint64_t chunk_bytes = after.index.bytes_written - before.index.bytes_written;
    laps.lap(3);

    // 6. Slots for all spans, then the table as an append builds it.
    if (n) {
        v = cdc::store_view(fs->store);
        if (nc) FL_TRY(cdc::launch_pack_slots(view, v.slot_of, fs->unpack.slot, s));
        FL_TRY(preset_stat(fs, s));
        FL_TRY(cdc::launch_files_append(made.t, 0, 0, fs->unpack.slot, v.length, v.loc, view.digest, n, fs->span.val,
                                        fs->span.block, &fs->dw->least, &fs->hw->appended, s));
        FL_TRY(fetch_stat(fs, s));
        FL_TRY(hipStreamSynchronize(s));
        made.n = n;
        made.size = fs->hw->appended;
        made.epoch = v.epoch;
        fold_stat(&made, fs->hw->least, fs->hw->zeros);
    }
    // The file's other spans are inserts of digests the store holds: a write of the content counts them too.
    cdc::store_count_written(fs->store, n - nc, made.size > chunk_bytes ? made.size - chunk_bytes : 0);
    fs->files[name] = new FileRec(made);
    guard.f = nullptr;
    laps.lap(4);
    std::memcpy(pack_split() + 2, laps.ms, 5 * sizeof(double));
    if (stats) {
        cdc_pack_stats_t r{};
        r.spans = n;
        r.chunks = nc;
        r.external_spans = h.external_spans;
        r.chunk_bytes = chunk_bytes;
        r.pack_bytes = h.total_bytes;
        r.file_size = made.size;
        r.chunks_new = (uint64_t)put;
        r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *stats = r;
    }
    return (int64_t)n;
}

}  // namespace

extern "C" {

int cdc_files_create(cdc_store_t *store, size_t seg_size, cdc_files_t **out) {
    if (!out) return fail(CDC_EINVAL, "cdc_files_create: out is NULL");
    *out = nullptr;
    if (!store) return fail(CDC_EINVAL, "cdc_files_create: store is NULL");
    cdc_files *fs = new cdc_files();
    fs->store = store;
    fs->seg = seg_size ? seg_size : (1u << 20);
    fs->device = cdc::store_view(store).device;
    hipError_t e = hipSetDevice(fs->device);
    if (e == hipSuccess) e = fs->hw.room(1);
    if (e == hipSuccess) e = fs->dw.room(1);
    if (e != hipSuccess) {
        delete fs;
        return fail_hip("cdc_files_create: ", e);
    }
    *out = fs;
    return CDC_OK;
}

void cdc_files_destroy(cdc_files_t *fs) {
    if (fs) release(fs);
}

int64_t cdc_files_clone(cdc_files_t *fs, const char *src, const char *dst, void *hip_stream) {
    if (!fs || !src || !dst) return fail(CDC_EINVAL, "cdc_files_clone: NULL argument");
    auto it = fs->files.find(src);
    if (it == fs->files.end()) return fail(CDC_ENOTFOUND, std::string("file layer: no file named '") + src + "'");
    const FileRec *from = it->second;
    int rc = check_epoch(fs, from, src);
    if (rc) return rc;
    if (fs->files.count(dst)) return fail(CDC_EEXIST, std::string("file layer: '") + dst + "' already exists");
    FileRec made = *from;  // n, size, epoch, min_len, zeros; the table is its own
    made.t = cdc::SpanTable{};
    made.cap = 0;
    if (from->n) {
        FL_TRY(hipSetDevice(cdc::store_view(fs->store).device));
        hipStream_t s = stream_of(fs, hip_stream);
        const uint64_t cap = table_cap(0, from->n);
        if ((rc = take_table(fs, cap, &made.t, "cdc_files_clone: span table: ")) != CDC_OK) return rc;
        hipError_t e = copy_spans(made.t, from->t, from->n, s);
        const hipError_t hs = hipStreamSynchronize(s);  // also on failure: nothing queued still writes the table
        if (e == hipSuccess) e = hs;
        if (e != hipSuccess) {
            fs->pool.give(made.t, cap);
            return fail_hip("cdc_files_clone: table copy: ", e);
        }
        made.cap = cap;
    }
    fs->files[dst] = new FileRec(made);
    return (int64_t)made.n;
}

int64_t cdc_files_diff_device(cdc_fh_t *a, cdc_fh_t *b, uint32_t flags, cdc_chunk_t *d_ranges, size_t cap,
                              cdc_diff_stats_t *stats, void *hip_stream) {
    const auto t0 = std::chrono::steady_clock::now();
    // Everything that can refuse, before any device work.
    if (flags & ~(uint32_t)CDC_DIFF_TABLES_ONLY)
        return fail(CDC_EINVAL, "cdc_files_diff_device: unknown flag bits " + std::to_string(flags));
    if (!a || !b) return fail(CDC_EINVAL, "cdc_files_diff_device: NULL file handle");
    if (cap && !d_ranges) return fail(CDC_EINVAL, "cdc_files_diff_device: NULL destination");
    if (a->fs && b->fs && a->fs != b->fs)
        return fail(CDC_EINVAL, "cdc_files_diff_device: the handles belong to two file layers");
    FileRec *fa = nullptr, *fb = nullptr;
    int rc = lookup(a, true, &fa);
    if (rc) return rc;
    if ((rc = lookup(b, true, &fb)) != CDC_OK) return rc;
    cdc_files *fs = a->fs;
    {
        cdc::ScrubView sv;
        bool stale = false;
        if (cdc::store_scrub_view(fs->store, &sv, &stale))
            return fail(CDC_ENOTSUP, "cdc_files_diff_device: the store holds target-kind containers (scrubbed); "
                                     "not supported");
    }
    const bool tables_only = (flags & CDC_DIFF_TABLES_ONLY) != 0;
    const uint64_t common = fa->size < fb->size ? fa->size : fb->size;
    const uint64_t maxsz = fa->size < fb->size ? fb->size : fa->size;
    const cdc::StoreView v = cdc::store_view(fs->store);
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    cdc_diff_stats_t r{};
    r.size_a = fa->size;
    r.size_b = fb->size;
    if (!common) {  // no byte to place in both files: the answer is the tail
        r.ranges = maxsz ? 1 : 0;
        r.bytes_differing = maxsz;
        if (r.ranges && r.ranges <= cap) {
            const cdc_chunk_t tail{0, maxsz};
            FL_TRY(hipMemcpyAsync(d_ranges, &tail, sizeof tail, hipMemcpyHostToDevice, s));
            FL_TRY(hipStreamSynchronize(s));
        }
    } else {
        cdc::DiffScratch w{};
        if ((rc = grow_diff(fs, fa->n, fb->n, common, tables_only, &w)) != CDC_OK) return rc;
        const cdc::DiffSide da{fa->t.off, fa->t.loc, fa->t.slot, fa->n, fa->size};
        const cdc::DiffSide db{fb->t.off, fb->t.loc, fb->t.slot, fb->n, fb->size};
        const hipError_t e = cdc::launch_files_diff(da, db, (uint64_t)(uintptr_t)v.arena, tables_only, w,
                                                    reinterpret_cast<cdc::cdc_chunk_pod *>(d_ranges), cap,
                                                    &fs->hw->ranges, s);
        const hipError_t hs = hipStreamSynchronize(s);  // the one wait of the call
        if (e != hipSuccess || hs != hipSuccess) {
            cdc::set_error(std::string("cdc_files_diff_device: ") + hipGetErrorString(e != hipSuccess ? e : hs));
            return CDC_EDEVICE;
        }
        r.ranges = fs->hw->ranges;
        r.bytes_differing = fs->hw->bytes_differing;
        r.bytes_compared = fs->hw->bytes_compared;
        r.bytes_shared = fs->hw->bytes_shared;
        r.pieces = fs->hw->pieces;
    }
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = r;
    return (int64_t)r.ranges;
}

int64_t cdc_files_delta_device(cdc_fh_t *a, cdc_fh_t *b, uint32_t flags, cdc_delta_op_t *d_ops, size_t cap,
                               cdc_delta_stats_t *stats, void *hip_stream) {
    const auto t0 = std::chrono::steady_clock::now();
    // Everything that can refuse, before any device work.
    if (flags & ~(uint32_t)CDC_DELTA_TABLES_ONLY)
        return fail(CDC_EINVAL, "cdc_files_delta_device: unknown flag bits " + std::to_string(flags));
    if (!a || !b) return fail(CDC_EINVAL, "cdc_files_delta_device: NULL file handle");
    if (cap && !d_ops) return fail(CDC_EINVAL, "cdc_files_delta_device: NULL destination");
    if (a->fs && b->fs && a->fs != b->fs)
        return fail(CDC_EINVAL, "cdc_files_delta_device: the handles belong to two file layers");
    FileRec *fa = nullptr, *fb = nullptr;
    int rc = lookup(a, true, &fa);
    if (rc) return rc;
    if ((rc = lookup(b, true, &fb)) != CDC_OK) return rc;
    cdc_files *fs = a->fs;
    if (scrubbed(fs))
        return fail(CDC_ENOTSUP, "cdc_files_delta_device: the store holds target-kind containers (scrubbed); "
                                 "not supported");
    const bool tables_only = (flags & CDC_DELTA_TABLES_ONLY) != 0;
    const cdc::StoreView v = cdc::store_view(fs->store);
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    cdc_delta_stats_t r{};
    r.size_a = fa->size;
    r.size_b = fb->size;
    if (!fb->size) {
        // no byte to build: no op
    } else if (!fa->size) {  // nothing to copy from: one LITERAL
        r.ops = r.regions = 1;
        r.bytes_literal = r.bytes_literal_tables = fb->size;
        if (cap) {
            const cdc_delta_op_t all{0, fb->size, CDC_DELTA_LITERAL};
            FL_TRY(hipMemcpyAsync(d_ops, &all, sizeof all, hipMemcpyHostToDevice, s));
            FL_TRY(hipStreamSynchronize(s));
        }
    } else {
        cdc::DeltaScratch w{};
        if ((rc = grow_delta(fs, fa->n, fb->n, fb->size, s, &w)) != CDC_OK) return rc;
        const cdc::DiffSide da{fa->t.off, fa->t.loc, fa->t.slot, fa->n, fa->size};
        const cdc::DiffSide db{fb->t.off, fb->t.loc, fb->t.slot, fb->n, fb->size};
        static_assert(sizeof(cdc::DeltaOp) == sizeof(cdc_delta_op_t), "one layout");
        const hipError_t e = cdc::launch_files_delta(da, db, (uint64_t)(uintptr_t)v.arena, tables_only, w,
                                                     reinterpret_cast<cdc::DeltaOp *>(d_ops), cap, fs->hw->delta, s);
        const hipError_t hs = hipStreamSynchronize(s);  // the one wait of the call
        if (e != hipSuccess || hs != hipSuccess) {
            cdc::set_error(std::string("cdc_files_delta_device: ") + hipGetErrorString(e != hipSuccess ? e : hs));
            return CDC_EDEVICE;
        }
        const word *h = fs->hw->delta;
        r.ops = h[0];
        r.bytes_copy = h[1];
        r.bytes_literal = h[2];
        r.bytes_literal_tables = h[3];
        r.spans_matched = h[4];
        r.regions = h[5];
    }
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = r;
    return (int64_t)r.ops;
}

int64_t cdc_file_pack_device(cdc_fh_t *fh, cdc_fh_t *since, const uint8_t *d_have, uint8_t *d_pack, size_t cap,
                             cdc_pack_stats_t *stats, void *hip_stream) {
    return pack_file(fh, since, d_have, d_pack, cap, stats, hip_stream);
}

int64_t cdc_files_unpack_device(cdc_files_t *fs, const char *name, const uint8_t *d_pack, size_t len,
                                cdc_handle_t *hasher, uint32_t flags, cdc_pack_stats_t *stats, void *hip_stream) {
    return unpack_file(fs, name, d_pack, len, hasher, flags, stats, hip_stream);
}

int cdc_debug_pack_split(double *ms, size_t n) {
    if (n && !ms) return fail(CDC_EINVAL, "cdc_debug_pack_split: NULL argument");
    if (n) std::memcpy(ms, pack_split(), (n < 7 ? n : 7) * sizeof(double));
    return 7;
}

int64_t cdc_debug_files_table_blocks(const cdc_files_t *fs) {
    if (!fs) return fail(CDC_EINVAL, "NULL file layer");
    return (int64_t)fs->pool.blocks.size();
}

int cdc_files_clear(cdc_files_t *fs) {
    if (!fs) return fail(CDC_EINVAL, "NULL file layer");
    (void)hipSetDevice(cdc::store_view(fs->store).device);
    drop_files(fs);
    return cdc_store_clear(fs->store);
}

int cdc_files_remove(cdc_files_t *fs, const char *name) {
    if (!fs || !name) return fail(CDC_EINVAL, "cdc_files_remove: NULL argument");
    auto it = fs->files.find(name);
    if (it == fs->files.end()) return fail(CDC_ENOTFOUND, std::string("file layer: no file named '") + name + "'");
    free_table(fs, it->second);
    delete it->second;
    fs->files.erase(it);  // handles hold the name: lookup() answers them with CDC_ENOTFOUND from here on
    return CDC_OK;
}

int cdc_files_collect(cdc_files_t *fs, cdc_collect_stats_t *out, void *hip_stream) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!fs) return fail(CDC_EINVAL, "NULL file layer");
    cdc::StoreView v = cdc::store_view(fs->store);
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    // The roots: every file whose spans were resolved under the store's present
    // epoch.  A file from before a clear names slots of another table.
    std::vector<FileRec *> roots;
    std::vector<cdc::CollectSeg> segs;
    std::vector<uint64_t> first{0};
    for (auto &kv : fs->files) {
        FileRec *f = kv.second;
        if (!f->n || f->epoch != v.epoch) continue;
        roots.push_back(f);
        segs.push_back(cdc::CollectSeg{f->t.slot, f->t.loc});
        first.push_back(first.back() + f->n);
    }
    const uint64_t nf = roots.size(), m = first.back();
    cdc::DeviceScratch mem;
    cdc::CollectSeg *d_seg = nullptr;
    uint64_t *d_first = nullptr;
    unsigned long long *refs = nullptr;
    uint32_t *map = nullptr;
    FL_TRY(mem.alloc(&d_seg, nf));
    FL_TRY(mem.alloc(&d_first, nf + 1));
    FL_TRY(mem.alloc(&refs, v.slots));
    FL_TRY(mem.alloc(&map, v.slots));
    FL_TRY(hipMemsetAsync(refs, 0, v.slots * 8, s));
    if (nf) FL_TRY(hipMemcpyAsync(d_seg, segs.data(), nf * sizeof(cdc::CollectSeg), hipMemcpyHostToDevice, s));
    FL_TRY(hipMemcpyAsync(d_first, first.data(), (nf + 1) * 8, hipMemcpyHostToDevice, s));
    FL_TRY(cdc::launch_files_refs(d_seg, d_first, nf, m, v.slots, refs, s));
    cdc_collect_stats_t r{};
    const int rc = cdc::store_retain(fs->store, refs, map, &r, s);  // waits for the stream
    if (rc) return rc;  // refused: no table was touched
    const auto t1 = std::chrono::steady_clock::now();
    v = cdc::store_view(fs->store);
    FL_TRY(cdc::launch_files_remap(d_seg, d_first, nf, m, v.slots, map, v.loc, s));
    FL_TRY(hipStreamSynchronize(s));
    for (FileRec *f : roots) f->epoch = v.epoch;
    cdc::collect_split()[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out) *out = r;
    return CDC_OK;
}

int cdc_files_exists(const cdc_files_t *fs, const char *name) {
    if (!fs || !name) return fail(CDC_EINVAL, "cdc_files_exists: NULL argument");
    return fs->files.count(name) ? 1 : 0;
}

int64_t cdc_files_list(const cdc_files_t *fs, char *buf, size_t cap) {
    if (!fs || (cap && !buf)) return fail(CDC_EINVAL, "cdc_files_list: NULL argument");
    uint64_t need = 0;
    for (const auto &kv : fs->files) need += kv.first.size() + 1;
    if (need > cap) return (int64_t)need;
    for (const auto &kv : fs->files) {
        std::memcpy(buf, kv.first.c_str(), kv.first.size() + 1);
        buf += kv.first.size() + 1;
    }
    return (int64_t)need;
}

int cdc_files_create_file(cdc_files_t *fs, const char *name, int create_new, cdc_fh_t **out) {
    if (!out) return fail(CDC_EINVAL, "cdc_files_create_file: out is NULL");
    *out = nullptr;
    if (!fs || !name) return fail(CDC_EINVAL, "cdc_files_create_file: NULL argument");
    auto it = fs->files.find(name);
    if (it != fs->files.end()) {
        if (!create_new) return fail(CDC_EEXIST, std::string("file layer: '") + name + "' already exists");
        (void)hipSetDevice(cdc::store_view(fs->store).device);
        free_table(fs, it->second);  // replaced by an empty file (file_layer.rs:95-96)
        *it->second = FileRec{};
    } else {
        fs->files[name] = new FileRec();
    }
    cdc_fh *fh = new cdc_fh();
    fh->fs = fs;
    fh->name = name;
    fs->handles.insert(fh);
    *out = fh;
    return CDC_OK;
}

int cdc_files_open(cdc_files_t *fs, const char *name, int readonly, cdc_fh_t **out) {
    if (!out) return fail(CDC_EINVAL, "cdc_files_open: out is NULL");
    *out = nullptr;
    if (!fs || !name) return fail(CDC_EINVAL, "cdc_files_open: NULL argument");
    if (!fs->files.count(name)) return fail(CDC_ENOTFOUND, std::string("file layer: no file named '") + name + "'");
    cdc_fh *fh = new cdc_fh();
    fh->fs = fs;
    fh->name = name;
    fh->readonly = readonly != 0;
    fs->handles.insert(fh);
    *out = fh;
    return CDC_OK;
}

void cdc_file_close(cdc_fh_t *fh) {
    if (!fh) return;
    if (fh->fs) fh->fs->handles.erase(fh);
    delete fh;
}

int cdc_file_stat(cdc_fh_t *fh, cdc_file_stat_t *out) {
    if (!out) return fail(CDC_EINVAL, "cdc_file_stat: out is NULL");
    FileRec *f = nullptr;
    const int rc = lookup(fh, false, &f);
    if (rc) return rc;
    out->size = f->size;
    out->spans = f->n;
    out->cursor = fh->cursor;
    out->chunk_seconds = fh->chunk_s;
    out->hash_seconds = fh->hash_s;
    return CDC_OK;
}

int64_t cdc_file_write_device(cdc_fh_t *fh, cdc_handle_t *chunker, const uint8_t *d_data, size_t len,
                              void *hip_stream) {
    FileRec *f = nullptr;
    int rc = lookup(fh, false, &f);
    if (rc) return rc;
    if (fh->readonly) return fail(CDC_EPERM, "file handle is read-only");
    if (!chunker) return fail(CDC_EINVAL, "cdc_file_write_device: NULL chunker");
    if (len == 0) return 0;
    if (!d_data) return fail(CDC_EINVAL, "cdc_file_write_device: NULL data");
    cdc_files *fs = fh->fs;
    FL_TRY(hipSetDevice(cdc::store_view(fs->store).device));
    void *s = hip_stream ? hip_stream : (void *)cdc::store_view(fs->store).stream;
    const uint64_t lens[1] = {len};
    const uint8_t *streams[1] = {d_data};
    const uint64_t cap = cdc_batch_max_chunks(chunker, 1, lens);
    FL_TRY(fs->wr.grow(cap));
    uint64_t first[2] = {0, 0};
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = cdc_chunk_batch_device(chunker, 1, streams, lens, fs->wr.chunks, cap, first, s);
    if (n < 0) return n;
    const auto t1 = std::chrono::steady_clock::now();
    rc = cdc_hash_batch_device(chunker, cdc_store_hash(fs->store), 1, streams, first, fs->wr.chunks, fs->wr.dig, s);
    if (rc) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    const int64_t got = append(fh, d_data, len, fs->wr.chunks, fs->wr.dig, (uint64_t)n, s);
    if (got < 0) return got;
    fh->chunk_s += std::chrono::duration<double>(t1 - t0).count();
    fh->hash_s += std::chrono::duration<double>(t2 - t1).count();
    return got;
}

int64_t cdc_file_append_device(cdc_fh_t *fh, const uint8_t *d_data, size_t data_len, const cdc_chunk_t *d_chunks,
                               const uint8_t *d_digests, size_t n, void *hip_stream) {
    return append(fh, d_data, data_len, d_chunks, d_digests, n, hip_stream);
}

int64_t cdc_file_splice_device(cdc_fh_t *fh, cdc_handle_t *chunker, uint64_t offset, uint64_t remove_len,
                               const uint8_t *d_data, size_t insert_len, cdc_splice_stats_t *out, void *hip_stream) {
    return splice(fh, chunker, offset, remove_len, d_data, insert_len, out, hip_stream);
}

int64_t cdc_debug_file_slots(cdc_fh_t *fh, uint32_t *slots, uint64_t *locs, size_t cap) {
    FileRec *f = nullptr;
    const int rc = lookup(fh, false, &f);
    if (rc) return rc;
    if (f->n > cap || f->n == 0) return (int64_t)f->n;
    FL_TRY(hipSetDevice(cdc::store_view(fh->fs->store).device));
    if (slots) FL_TRY(hipMemcpy(slots, f->t.slot, f->n * 4, hipMemcpyDeviceToHost));
    if (locs) FL_TRY(hipMemcpy(locs, f->t.loc, f->n * 8, hipMemcpyDeviceToHost));
    return (int64_t)f->n;
}

int cdc_debug_splice_split(double *ms, size_t n) {
    if (n && !ms) return fail(CDC_EINVAL, "cdc_debug_splice_split: NULL argument");
    if (n) std::memcpy(ms, splice_split(), (n < 5 ? n : 5) * sizeof(double));
    return 5;
}

int64_t cdc_files_write_batch_device(cdc_files_t *fs, cdc_handle_t *chunker, size_t n, const cdc_fwrite_t *reqs,
                                     uint64_t *spans, void *hip_stream) {
    if (!fs) return fail(CDC_EINVAL, "NULL file layer");
    if (!chunker) return fail(CDC_EINVAL, "cdc_files_write_batch_device: NULL chunker");
    if (n == 0) return 0;
    if (!reqs) return fail(CDC_EINVAL, "cdc_files_write_batch_device: NULL argument");
    // Everything that can refuse, before the store or a table's contents are touched.
    cdc::StoreView v = cdc::store_view(fs->store);
    std::vector<FileRec *> recs(n);
    std::set<FileRec *> seen;
    std::vector<const uint8_t *> streams;
    std::vector<uint64_t> lens;
    uint64_t bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        cdc_fh *fh = reqs[i].fh;
        if (fh && fh->fs && fh->fs != fs)
            return fail(CDC_EINVAL, "cdc_files_write_batch_device: a handle of another layer");
        const int rc = writable(fh, &recs[i]);
        if (rc) return rc;
        if (reqs[i].len && !reqs[i].d_data) return fail(CDC_EINVAL, "cdc_files_write_batch_device: NULL data");
        if (!seen.insert(recs[i]).second)
            return fail(CDC_EINVAL, "cdc_files_write_batch_device: '" + fh->name + "' is named twice");
        if (reqs[i].len) {  // a request without bytes is no stream: it appends nothing
            streams.push_back(reqs[i].d_data);
            lens.push_back(reqs[i].len);
            bytes += reqs[i].len;
        }
    }
    const size_t ns = streams.size();
    if (ns == 0) {
        if (spans) std::memset(spans, 0, n * sizeof(uint64_t));
        return 0;
    }
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    const uint64_t cap = cdc_batch_max_chunks(chunker, ns, lens.data());
    FL_TRY(fs->wr.grow(cap));
    std::vector<uint64_t> sfirst(ns + 1, 0);
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t m = cdc_chunk_batch_device(chunker, ns, streams.data(), lens.data(), fs->wr.chunks, cap,
                                             sfirst.data(), s);
    if (m < 0) return m;
    const auto t1 = std::chrono::steady_clock::now();
    int rc = cdc_hash_batch_device(chunker, cdc_store_hash(fs->store), ns, streams.data(), sfirst.data(), fs->wr.chunks, fs->wr.dig, s);
    if (rc) return rc;
    const auto t2 = std::chrono::steady_clock::now();

    // Room for every file's new spans (the contents stay as they are), then the one put.
    FL_TRY(fs->batch.grow(n));
    FL_TRY(fs->span.grow((uint64_t)m));
    uint64_t *h_first = reinterpret_cast<uint64_t *>(fs->batch.h.p);
    cdc::AppendDst *h_dst = reinterpret_cast<cdc::AppendDst *>(h_first + n + 1);
    cdc::AppendStat *h_stat = reinterpret_cast<cdc::AppendStat *>(h_dst + n);
    bool copied = false;
    h_first[0] = 0;
    for (size_t i = 0, j = 0; i < n; ++i) {
        const uint64_t cnt = reqs[i].len ? sfirst[j + 1] - sfirst[j] : 0;
        if (reqs[i].len) ++j;
        h_first[i + 1] = h_first[i] + cnt;
        if (cnt && (rc = reserve(fs, recs[i], recs[i]->n + cnt, s, &copied)) != CDC_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
    }
    if (copied) FL_TRY(hipStreamSynchronize(s));
    const int64_t put = cdc::store_put_batch_slots(fs->store, ns, streams.data(), lens.data(), sfirst.data(),
                                                   fs->wr.chunks, fs->wr.dig, s);
    if (put < 0) return put;  // refused: every file is as it was
    v = cdc::store_view(fs->store);
    for (size_t i = 0; i < n; ++i) {
        h_dst[i] = cdc::AppendDst{recs[i]->t, recs[i]->n, recs[i]->size};
        h_stat[i] = cdc::AppendStat{0, ~0ull, 0};
    }
    uint64_t *d_first = reinterpret_cast<uint64_t *>(fs->batch.d.p);
    cdc::AppendDst *d_dst = reinterpret_cast<cdc::AppendDst *>(d_first + n + 1);
    cdc::AppendStat *d_stat = reinterpret_cast<cdc::AppendStat *>(d_dst + n);
    FL_TRY(hipMemcpyAsync(fs->batch.d, fs->batch.h, batch_bytes(n), hipMemcpyHostToDevice, s));
    FL_TRY(cdc::launch_files_append_batch(d_dst, d_first, n, (uint64_t)m, v.slot_of, v.length, v.loc, fs->wr.dig,
                                          fs->span.val, fs->span.block, d_stat, s));
    FL_TRY(hipMemcpyAsync(h_stat, d_stat, n * sizeof(cdc::AppendStat), hipMemcpyDeviceToHost, s));
    FL_TRY(hipStreamSynchronize(s));
    const double chunk_s = std::chrono::duration<double>(t1 - t0).count();
    const double hash_s = std::chrono::duration<double>(t2 - t1).count();
    for (size_t i = 0; i < n; ++i) {
        const uint64_t cnt = h_first[i + 1] - h_first[i];
        const double share = (double)reqs[i].len / (double)bytes;
        reqs[i].fh->chunk_s += chunk_s * share;
        reqs[i].fh->hash_s += hash_s * share;
        if (spans) spans[i] = cnt;
        if (!cnt) continue;
        FileRec *f = recs[i];
        f->n += cnt;
        f->size += h_stat[i].bytes;
        f->epoch = v.epoch;
        fold_stat(f, h_stat[i].least, h_stat[i].zeros);
    }
    return m;
}

int64_t cdc_file_read_complete_device(cdc_fh_t *fh, uint8_t *d_out, size_t out_cap, cdc_chunk_t *d_spans,
                                      void *hip_stream) {
    return read_one(fh, cdc::kReadComplete, 0, 0, d_out, out_cap, d_spans, hip_stream);
}

int64_t cdc_file_read_device(cdc_fh_t *fh, uint8_t *d_out, size_t out_cap, void *hip_stream) {
    if (!fh || !fh->fs) return fail(CDC_EINVAL, "NULL file handle");
    const int64_t got = read_one(fh, cdc::kReadSegment, fh->cursor, fh->fs->seg, d_out, out_cap, nullptr, hip_stream);
    if (got > 0 && (uint64_t)got <= out_cap) fh->cursor += (uint64_t)got;  // handle.offset += bytes_read
    return got;
}

int64_t cdc_file_pread_device(cdc_fh_t *fh, uint64_t offset, size_t len, uint8_t *d_out, void *hip_stream) {
    return read_one(fh, cdc::kReadRange, offset, len, d_out, len, nullptr, hip_stream);
}

int cdc_files_pread_batch_device(cdc_files_t *fs, size_t n, const cdc_pread_t *reqs, uint64_t *got,
                                 void *hip_stream) {
    if (!fs) return fail(CDC_EINVAL, "NULL file layer");
    if (n == 0) return CDC_OK;
    if (!reqs || !got) return fail(CDC_EINVAL, "cdc_files_pread_batch_device: NULL argument");
    std::vector<HostReq> v;
    v.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        FileRec *f = nullptr;
        const int rc = lookup(reqs[i].fh, true, &f);
        if (rc) return rc;
        if (reqs[i].fh->fs != fs) return fail(CDC_EINVAL, "cdc_files_pread_batch_device: a handle of another layer");
        if (reqs[i].len && !reqs[i].d_dst) return fail(CDC_EINVAL, "cdc_files_pread_batch_device: NULL destination");
        v.push_back(HostReq{f, cdc::kReadRange, reqs[i].offset, reqs[i].len, reqs[i].d_dst, reqs[i].len,
                            nullptr});
    }
    const int rc = run_reads(fs, v, hip_stream);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) got[i] = fs->req.h_res[i].bytes;
    return CDC_OK;
}

int64_t cdc_file_hashes_device(cdc_fh_t *fh, uint8_t *d_digests, size_t cap) {
    FileRec *f = nullptr;
    const int rc = lookup(fh, false, &f);
    if (rc) return rc;
    if (f->n > cap || f->n == 0) return (int64_t)f->n;
    if (!d_digests) return fail(CDC_EINVAL, "cdc_file_hashes_device: NULL destination");
    const cdc::StoreView v = cdc::store_view(fh->fs->store);
    FL_TRY(hipSetDevice(v.device));
    FL_TRY(hipMemcpyAsync(d_digests, f->t.digest, f->n * 32, hipMemcpyDeviceToDevice, v.stream));
    FL_TRY(hipStreamSynchronize(v.stream));
    return (int64_t)f->n;
}

int64_t cdc_file_distribution_device(cdc_fh_t *fh, uint8_t *d_digests, uint32_t *d_counts, uint64_t *d_lengths,
                                     size_t cap, void *hip_stream) {
    FileRec *f = nullptr;
    int rc = lookup(fh, true, &f);
    if (rc) return rc;
    if (f->n < 2) return 0;  // the zip with skip(1) drops the last span
    if (cap && (!d_digests || !d_counts || !d_lengths))
        return fail(CDC_EINVAL, "cdc_file_distribution_device: NULL destination");
    cdc_files *fs = fh->fs;
    const cdc::StoreView v = cdc::store_view(fs->store);
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);
    const uint64_t m = f->n - 1;
    FL_TRY(fs->span.grow(m));
    FL_TRY(fs->slot.grow(v.slots));
    FL_TRY(cdc::launch_files_distribution(f->t, m, fs->slot.cnt, fs->slot.first, fs->span.val, fs->span.block,
                                          d_digests, d_counts, d_lengths, cap, &fs->hw->distinct, s));
    FL_TRY(hipStreamSynchronize(s));
    return (int64_t)fs->hw->distinct;
}

int64_t cdc_file_verify_device(cdc_fh_t *fh, const uint8_t *d_data, size_t len, uint64_t *first_diff,
                               void *hip_stream) {
    FileRec *f = nullptr;
    int rc = lookup(fh, true, &f);
    if (rc) return rc;
    if (len && !d_data) return fail(CDC_EINVAL, "cdc_file_verify_device: NULL data");
    const uint64_t common = f->size < len ? f->size : (uint64_t)len;
    uint64_t diff = ~0ull;
    if (common) {
        // The planner's range read of [0, common) with the dataset as its "destination": pieces past the shorter
        // of the two never exist, so the compare stays inside [d_data, d_data + len).
        std::vector<HostReq> reqs{
            HostReq{f, cdc::kReadRange, 0, common, const_cast<uint8_t *>(d_data), common, nullptr}};
        if ((rc = run_reads(fh->fs, reqs, hip_stream, d_data)) != CDC_OK) return rc;
        diff = fh->fs->hw->verify;
    }
    if (diff == ~0ull && f->size != len) diff = common;
    if (first_diff) *first_diff = diff;
    return diff == ~0ull ? 1 : 0;
}

int64_t cdc_files_get_to_dedup_ratio(cdc_files_t *fs, const char *name, double dedup_ratio, char *out_name,
                                     size_t out_cap, void *hip_stream) {
    if (!fs || !name || (out_cap && !out_name))
        return fail(CDC_EINVAL, "cdc_files_get_to_dedup_ratio: NULL argument");
    if (!(dedup_ratio >= 1.0)) return fail(CDC_EINVAL, "dedup ratio must be bigger than 1");  // NaN too
    if (!std::isfinite(dedup_ratio)) return fail(CDC_EINVAL, "cdc_files_get_to_dedup_ratio: the ratio is not finite");
    auto it = fs->files.find(name);
    if (it == fs->files.end()) return fail(CDC_ENOTFOUND, std::string("file with name `") + name + "` not found");
    FileRec *src = it->second;
    int rc = check_epoch(fs, src, name);
    if (rc) return rc;
    const cdc::StoreView v = cdc::store_view(fs->store);
    char suffix[400];  // "%.2f" of the largest double has 312 characters
    std::snprintf(suffix, sizeof suffix, ".%.2f", dedup_ratio);
    const std::string new_name = std::string(name) + suffix;
    FL_TRY(hipSetDevice(v.device));
    hipStream_t s = stream_of(fs, hip_stream);

    cdc::DeviceScratch mem;
    FileRec made;  // the new file; its table is freed again unless the call succeeds
    made.epoch = src->epoch;
    struct Guard {
        cdc_files *fs;
        FileRec *f;
        ~Guard() {
            if (f) free_table(fs, f);
        }
    } guard{fs, &made};
    if (src->n >= 2) {
        // 1. The unique list over all but the last span (the reference's zip with skip(1)).
        const uint64_t m = src->n - 1;
        FL_TRY(fs->span.grow(m));
        FL_TRY(fs->slot.grow(v.slots));
        uint64_t *uidx = nullptr, *ulen = nullptr, *ublock = nullptr, *sidx = nullptr;
        FL_TRY(mem.alloc(&uidx, m));
        FL_TRY(mem.alloc(&ulen, m));
        FL_TRY(mem.alloc(&ublock, cdc::store_scan_blocks(m) + 1));
        FL_TRY(cdc::launch_files_ratio_unique(src->t, m, fs->slot.cnt, fs->slot.first, fs->span.val, fs->span.block,
                                              uidx, ulen, ublock, &fs->hw->unique, s));
        FL_TRY(hipStreamSynchronize(s));
        const uint64_t U = fs->hw->unique, unique_length = fs->hw->unique_length;
        if (U) {
            // 2. file_layer.rs:233-237, in f64 as written there (`as usize` saturates).
            const double want = (double)unique_length * dedup_ratio;
            const uint64_t total_size = want >= 18446744073709551616.0 ? ~0ull : (uint64_t)want;
            const double rep = std::ceil((double)U * (1.0 / dedup_ratio));
            uint64_t R = rep >= 18446744073709551616.0 ? ~0ull : (uint64_t)rep;
            if (R > U) R = U;  // take(num_repeating) of U entries
            uint64_t K = 0;
            if (R) {
                FL_TRY(cdc::launch_files_ratio_take(ulen, ublock, m, R, total_size, &fs->hw->cycle, s));
                FL_TRY(hipStreamSynchronize(s));
                const uint64_t C = fs->hw->cycle, j = fs->hw->partial;
                if (C == 0)
                    return fail(CDC_EINVAL, "cdc_files_get_to_dedup_ratio: the repeating spans are all empty "
                                            "(the reference's cycle would never end)");
                if (__builtin_mul_overflow(total_size / C, R, &K) || __builtin_add_overflow(K, j, &K))
                    return fail(CDC_ENOMEM, "cdc_files_get_to_dedup_ratio: the new span table cannot be allocated");
            }
            uint64_t n = 0;
            if (__builtin_add_overflow(K, U - R, &n) || n > (1ull << 40))
                return fail(CDC_ENOMEM, "cdc_files_get_to_dedup_ratio: the new span table cannot be allocated");
            // 3. The new table: gather, scan, write.
            if (n) {
                if ((rc = reserve(fs, &made, n, s)) != CDC_OK) return rc;
                FL_TRY(fs->span.grow(n));
                FL_TRY(mem.alloc(&sidx, n));
                FL_TRY(preset_stat(fs, s));
                FL_TRY(cdc::launch_files_ratio_gather(src->t, made.t, uidx, K, R, n, sidx, fs->span.val, fs->span.block,
                                                      &fs->dw->least, &fs->hw->appended, s));
                FL_TRY(fetch_stat(fs, s));
                FL_TRY(hipStreamSynchronize(s));
                made.n = n;
                made.size = fs->hw->appended;
                fold_stat(&made, fs->hw->least, fs->hw->zeros);
            }
        }
    }
    // HashMap::insert (file_layer.rs:265): the name's old file, if any, is replaced.
    FileRec *&slot = fs->files[new_name];
    if (slot) free_table(fs, slot);
    else slot = new FileRec();
    *slot = made;
    guard.f = nullptr;
    const size_t need = new_name.size() + 1;
    if (need <= out_cap) std::memcpy(out_name, new_name.c_str(), need);
    return (int64_t)need;
}

}  // extern "C"
