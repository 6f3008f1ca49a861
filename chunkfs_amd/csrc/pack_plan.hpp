// pack_plan.hpp -- the arithmetic of cdc_file_pack_device and
// cdc_files_unpack_device (include/chunkfs_amd.h, "Packs"), header-only and free
// of HIP so that a plain C++ program can run it under the host sanitizers
// (tools/pack_plan_check.cpp).  pack.hip uses the same functions on the device.
//
// Three things live here: the header and the section offsets of a pack with the
// overflow-free recomputation of its size; the host's header check; and the
// predicates of the validation kernel, each of which reads an index section
// only at positions it has bounded itself -- a pack is untrusted input.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CDC_PACK_HD __host__ __device__ __forceinline__
#else
#define CDC_PACK_HD inline
#endif

namespace cdc {

constexpr uint64_t kPackMagic = 0x314B434150434443ull;  // the bytes "CDCPACK1", little-endian
constexpr uint32_t kPackVersion = 1;
constexpr uint64_t kPackAlign = 16;        // sections and carried chunks start at multiples of it
constexpr uint64_t kPackHeaderBytes = 64;
constexpr uint64_t kPackExternal = ~0ull;  // span_chunk of a span whose chunk the pack does not carry

struct PackHeader {
    uint64_t magic;
    uint32_t version, flags;
    uint64_t file_size, n_spans, n_chunks, external_spans, data_bytes, total_bytes;
};
static_assert(sizeof(PackHeader) == kPackHeaderBytes, "the header is 64 bytes");

// The flags word: bits 0-7 carry the hasher of the pack's digests (CDC_HASH_*:
// 0 is SHA-256, so a default store's pack has flags 0); every other bit is 0.
constexpr uint32_t kPackHashMask = 0xFFu;
CDC_PACK_HD uint32_t pack_flags(uint32_t hash) { return hash & kPackHashMask; }

// Byte offsets of the sections from the start of the pack.
struct PackLayout {
    uint64_t digest, length, span_chunk, chunk_span, chunk_off, data, total;
};

// round_up(x, 16); false when it passes 2^64.
CDC_PACK_HD bool pack_pad(uint64_t x, uint64_t *out) {
    if (x > ~0ull - (kPackAlign - 1)) return false;
    *out = (x + (kPackAlign - 1)) & ~(kPackAlign - 1);
    return true;
}

// *at += round_up(count * width, 16), false when either step passes 2^64.
CDC_PACK_HD bool pack_section(uint64_t count, uint64_t width, uint64_t *at) {
    uint64_t bytes = 0;
    if (width && count > ~0ull / width) return false;
    if (!pack_pad(count * width, &bytes)) return false;
    if (*at > ~0ull - bytes) return false;
    *at += bytes;
    return true;
}

// The section offsets of a pack of n_spans spans and n_chunks carried chunks
// whose data section has data_bytes bytes; false when a size passes 2^64.  A
// pack without spans has no sections at all.
CDC_PACK_HD bool pack_layout(uint64_t n_spans, uint64_t n_chunks, uint64_t data_bytes, PackLayout *out) {
    if (n_chunks == ~0ull) return false;  // chunk_off has n_chunks + 1 entries
    uint64_t at = kPackHeaderBytes;
    if (n_spans == 0) {  // an empty file is its header: no section, not even chunk_off[0]
        if (n_chunks || data_bytes) return false;
        out->digest = out->length = out->span_chunk = out->chunk_span = out->chunk_off = out->data = out->total = at;
        return true;
    }
    out->digest = at;
    if (!pack_section(n_spans, 32, &at)) return false;
    out->length = at;
    if (!pack_section(n_spans, 8, &at)) return false;
    out->span_chunk = at;
    if (!pack_section(n_spans, 8, &at)) return false;
    out->chunk_span = at;
    if (!pack_section(n_chunks, 8, &at)) return false;
    out->chunk_off = at;
    if (!pack_section(n_chunks + 1, 8, &at)) return false;
    out->data = at;
    if (!pack_section(data_bytes, 1, &at)) return false;
    out->total = at;
    return true;
}

// The checks of an unpack in the order they run; cdc_last_error() names them.
enum PackCheck : uint32_t {
    kPackOk = 0,
    kPackMagicCheck,      // host: the header
    kPackVersionCheck,
    kPackFlagsCheck,
    kPackSizesCheck,      // a section size passes 2^64, n_chunks > n_spans, data_bytes is no multiple of 16
    kPackTotalCheck,      // total_bytes is not what n_spans / n_chunks / data_bytes give
    kPackLenCheck,        // total_bytes > len
    kPackChunkSpanCheck,  // device: chunk_span strictly increasing and < n_spans
    kPackSpanChunkCheck,  // span_chunk[i] == ~0 or < n_chunks
    kPackBackrefCheck,    // span_chunk[chunk_span[k]] == k
    kPackSameCheck,       // a carried span equals the first span of its chunk in digest and length
    kPackChunkOffCheck,   // chunk_off[0] == 0, steps of round_up(length, 16)
    kPackDataBytesCheck,  // chunk_off[n_chunks] == data_bytes
    kPackFileSizeCheck,   // the lengths sum to file_size
    kPackExternalCheck,   // external_spans counts the ~0 entries
    kPackChecks
};
constexpr uint32_t kPackFirstDeviceCheck = kPackChunkSpanCheck;

CDC_PACK_HD const char *pack_check_name(uint32_t c) {
    switch (c) {
        case kPackMagicCheck: return "magic";
        case kPackVersionCheck: return "version";
        case kPackFlagsCheck: return "flags";
        case kPackSizesCheck: return "section sizes";
        case kPackTotalCheck: return "total_bytes";
        case kPackLenCheck: return "length";
        case kPackChunkSpanCheck: return "chunk_span order";
        case kPackSpanChunkCheck: return "span_chunk range";
        case kPackBackrefCheck: return "span_chunk of a first occurrence";
        case kPackSameCheck: return "span equals its chunk";
        case kPackChunkOffCheck: return "chunk_off steps";
        case kPackDataBytesCheck: return "data_bytes";
        case kPackFileSizeCheck: return "file_size";
        case kPackExternalCheck: return "external_spans";
        default: return "ok";
    }
}

// The host's check of a header read from a pack of `len` bytes (len >= 64).
// On kPackOk *out holds the section offsets, every one of them <= len.
// `hash`: the receiving store's hasher (CDC_HASH_*), which the pack must name.
CDC_PACK_HD uint32_t pack_check_header(const PackHeader &h, uint64_t len, PackLayout *out, uint32_t hash = 0) {
    if (h.magic != kPackMagic) return kPackMagicCheck;
    if (h.version != kPackVersion) return kPackVersionCheck;
    if (h.flags != pack_flags(hash)) return kPackFlagsCheck;
    if (h.n_chunks > h.n_spans || (h.data_bytes & (kPackAlign - 1))) return kPackSizesCheck;
    if (!pack_layout(h.n_spans, h.n_chunks, h.data_bytes, out)) return kPackSizesCheck;
    if (out->total != h.total_bytes) return kPackTotalCheck;
    if (h.total_bytes > len) return kPackLenCheck;
    return kPackOk;
}

// The index sections of a pack whose header passed pack_check_header: every
// array holds the number of entries the header states.
struct PackView {
    const uint8_t *digest;       // [n_spans * 32]
    const uint64_t *length;      // [n_spans]
    const uint64_t *span_chunk;  // [n_spans]
    const uint64_t *chunk_span;  // [n_chunks]
    const uint64_t *chunk_off;   // [n_chunks + 1]
    uint64_t n_spans, n_chunks, data_bytes, file_size, external_spans;
};

CDC_PACK_HD PackView pack_view(const uint8_t *pack, const PackHeader &h, const PackLayout &l) {
    PackView v;
    v.digest = pack + l.digest;
    v.length = reinterpret_cast<const uint64_t *>(pack + l.length);
    v.span_chunk = reinterpret_cast<const uint64_t *>(pack + l.span_chunk);
    v.chunk_span = reinterpret_cast<const uint64_t *>(pack + l.chunk_span);
    v.chunk_off = reinterpret_cast<const uint64_t *>(pack + l.chunk_off);
    v.n_spans = h.n_spans;
    v.n_chunks = h.n_chunks;
    v.data_bytes = h.data_bytes;
    v.file_size = h.file_size;
    v.external_spans = h.external_spans;
    return v;
}

// The predicates.  k < n_chunks and i < n_spans are the caller's; every other
// index is bounded here before it is used, and a predicate whose index is out of
// range holds: the check that bounds that index reports it.

CDC_PACK_HD bool pack_ok_chunk_span(const PackView &v, uint64_t k) {
    const uint64_t i = v.chunk_span[k];
    return i < v.n_spans && (k == 0 || v.chunk_span[k - 1] < i);
}

CDC_PACK_HD bool pack_ok_span_chunk(const PackView &v, uint64_t i) {
    const uint64_t c = v.span_chunk[i];
    return c == kPackExternal || c < v.n_chunks;
}

CDC_PACK_HD bool pack_ok_backref(const PackView &v, uint64_t k) {
    const uint64_t i = v.chunk_span[k];
    return i >= v.n_spans || v.span_chunk[i] == k;
}

CDC_PACK_HD bool pack_ok_same(const PackView &v, uint64_t i) {
    const uint64_t c = v.span_chunk[i];
    if (c == kPackExternal || c >= v.n_chunks) return true;
    const uint64_t j = v.chunk_span[c];
    if (j >= v.n_spans) return true;
    if (v.length[i] != v.length[j]) return false;
    for (uint32_t b = 0; b < 32; ++b)
        if (v.digest[32 * i + b] != v.digest[32 * j + b]) return false;
    return true;
}

// chunk_off[k + 1] - chunk_off[k] == round_up(length of chunk k, 16), and the
// first entry is 0.  Entries that decrease fail, whatever the difference wraps to.
CDC_PACK_HD bool pack_ok_chunk_off(const PackView &v, uint64_t k) {
    if (k == 0 && v.chunk_off[0] != 0) return false;
    const uint64_t i = v.chunk_span[k];
    if (i >= v.n_spans) return true;
    uint64_t padded = 0;
    if (!pack_pad(v.length[i], &padded)) return false;
    const uint64_t a = v.chunk_off[k], b = v.chunk_off[k + 1];
    return b >= a && b - a == padded;
}

CDC_PACK_HD bool pack_ok_data_bytes(const PackView &v) {
    if (v.n_spans == 0) return true;  // no chunk_off section
    return v.chunk_off[v.n_chunks] == v.data_bytes && (v.n_chunks || v.chunk_off[0] == 0);
}

// A sum of lengths that cannot wrap unnoticed: the low 64 bits and how often
// they passed 2^64.
struct PackSum {
    uint64_t low, wraps;
};
CDC_PACK_HD PackSum pack_sum_add(PackSum a, PackSum b) {
    PackSum r;
    r.low = a.low + b.low;
    r.wraps = a.wraps + b.wraps + (r.low < a.low ? 1 : 0);
    return r;
}
CDC_PACK_HD bool pack_ok_file_size(const PackView &v, PackSum lengths) {
    return lengths.wraps == 0 && lengths.low == v.file_size;
}

}  // namespace cdc
