// pack_plan_check.cpp -- the arithmetic of cdc_file_pack_device and
// cdc_files_unpack_device (chunkfs_amd/csrc/pack_plan.hpp) against brute force,
// as a plain C++ program for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I chunkfs_amd/csrc tools/pack_plan_check.cpp -o pack_plan_check && ./pack_plan_check
// Every index section is a heap array of exactly the entries the header states,
// so a predicate that follows an index it has not bounded is an error the
// sanitizer reports.  Exit code 0 and "pack plan ok" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pack_plan.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
            ++failures;                                               \
        }                                                             \
    } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

typedef unsigned __int128 u128;
const u128 kLimit = (u128)1 << 64;

u128 pad(u128 x) { return (x + 15) / 16 * 16; }

// The layout in 128-bit arithmetic: false when the total does not fit 64 bits.
bool brute_layout(uint64_t n, uint64_t nc, uint64_t data, u128 out[7]) {
    if (n == 0) {
        for (int i = 0; i < 7; ++i) out[i] = 64;
        return nc == 0 && data == 0;
    }
    const u128 sizes[6] = {(u128)n * 32, (u128)n * 8, (u128)n * 8, (u128)nc * 8, ((u128)nc + 1) * 8, (u128)data};
    u128 at = 64;
    for (int i = 0; i < 6; ++i) {
        out[i] = at;
        at += pad(sizes[i]);
    }
    out[6] = at;
    return at < kLimit;
}

void check_layout_one(uint64_t n, uint64_t nc, uint64_t data) {
    u128 want[7];
    cdc::PackLayout l{};
    const bool ok = brute_layout(n, nc, data, want), got = cdc::pack_layout(n, nc, data, &l);
    CHECK(ok == got);
    if (!ok || !got) return;
    const uint64_t have[7] = {l.digest, l.length, l.span_chunk, l.chunk_span, l.chunk_off, l.data, l.total};
    for (int i = 0; i < 7; ++i) {
        CHECK((u128)have[i] == want[i]);
        CHECK(have[i] % 16 == 0);
    }
}

void check_layout() {
    const uint64_t edge[] = {0, 1, 2, 3, 15, 16, 17, 2048, 2049, (1ull << 27) - 1, 1ull << 27, (1ull << 29) + 1,
                             1ull << 32, (1ull << 32) + 1, 1ull << 56, (1ull << 59) - 1, 1ull << 59, (1ull << 59) + 1,
                             1ull << 60, (1ull << 61) - 1, 1ull << 61, 1ull << 63, ~0ull - 16, ~0ull - 15, ~0ull - 1,
                             ~0ull};
    const size_t ne = sizeof edge / sizeof edge[0];
    for (size_t a = 0; a < ne; ++a)
        for (size_t b = 0; b < ne; ++b)
            for (size_t c = 0; c < ne; ++c) check_layout_one(edge[a], edge[b], edge[c]);
    for (int t = 0; t < 20000; ++t) {
        const uint64_t n = rnd() >> (rnd() % 64), nc = rnd() >> (rnd() % 64), d = rnd() >> (rnd() % 64);
        check_layout_one(n, nc, d);
    }
    // Sizes whose bytes exceed 2^32 are laid out, those that wrap 2^64 are refused, not wrapped.
    cdc::PackLayout l{};
    CHECK(cdc::pack_layout(1ull << 28, 1ull << 28, 1ull << 33, &l) && l.total > (1ull << 32));
    CHECK(!cdc::pack_layout(1ull << 59, 0, 0, &l));   // 32 * n_spans = 2^64
    CHECK(!cdc::pack_layout(1ull << 61, 0, 0, &l));
    CHECK(!cdc::pack_layout(1, ~0ull, 0, &l));         // n_chunks + 1 wraps
    CHECK(!cdc::pack_layout(1, 1, ~0ull - 7, &l));     // round_up(data_bytes) wraps
    CHECK(!cdc::pack_layout(1, 1, ~0ull - 100, &l));   // the sum wraps
    CHECK(!cdc::pack_layout(0, 1, 0, &l) && !cdc::pack_layout(0, 0, 16, &l));
    CHECK(cdc::pack_layout(0, 0, 0, &l) && l.total == 64 && l.data == 64);
    uint64_t p = 0;
    CHECK(cdc::pack_pad(0, &p) && p == 0);
    CHECK(cdc::pack_pad(1, &p) && p == 16);
    CHECK(cdc::pack_pad(16, &p) && p == 16);
    CHECK(cdc::pack_pad(17, &p) && p == 32);
    CHECK(cdc::pack_pad(~0ull - 15, &p) && p == ~0ull - 15);
    CHECK(!cdc::pack_pad(~0ull - 14, &p) && !cdc::pack_pad(~0ull, &p));
}

void check_header() {
    cdc::PackLayout l{};
    cdc::pack_layout(5, 3, 64, &l);
    const cdc::PackHeader good{cdc::kPackMagic, 1, 0, 100, 5, 3, 0, 64, l.total};
    cdc::PackLayout got{};
    CHECK(cdc::pack_check_header(good, l.total, &got) == cdc::kPackOk && got.total == l.total);
    CHECK(cdc::pack_check_header(good, l.total + 100, &got) == cdc::kPackOk);
    CHECK(cdc::pack_check_header(good, l.total - 1, &got) == cdc::kPackLenCheck);
    cdc::PackHeader h = good;
    h.magic ^= 1;
    CHECK(cdc::pack_check_header(h, l.total, &got) == cdc::kPackMagicCheck);
    h = good, h.version = 2;
    CHECK(cdc::pack_check_header(h, l.total, &got) == cdc::kPackVersionCheck);
    h = good, h.flags = 1;
    CHECK(cdc::pack_check_header(h, l.total, &got) == cdc::kPackFlagsCheck);
    // The hasher in bits 0-7: accepted by a receiver with the same hasher only,
    // and no other bit may be set.
    CHECK(cdc::pack_flags(0) == 0 && cdc::pack_flags(1) == 1);
    CHECK(cdc::pack_check_header(h, l.total, &got, 1) == cdc::kPackOk && got.total == l.total);
    CHECK(cdc::pack_check_header(good, l.total, &got, 0) == cdc::kPackOk);
    CHECK(cdc::pack_check_header(good, l.total, &got, 1) == cdc::kPackFlagsCheck);
    CHECK(cdc::pack_check_header(h, l.total, &got, 0) == cdc::kPackFlagsCheck);
    for (uint32_t bit = 8; bit < 32; ++bit) {
        h = good, h.flags = 1u << bit;
        CHECK(cdc::pack_check_header(h, l.total, &got, 0) == cdc::kPackFlagsCheck);
        h.flags |= 1;
        CHECK(cdc::pack_check_header(h, l.total, &got, 1) == cdc::kPackFlagsCheck);
        CHECK(cdc::pack_check_header(h, l.total, &got, 0) == cdc::kPackFlagsCheck);
    }
    h = good, h.n_chunks = 6;
    CHECK(cdc::pack_check_header(h, l.total, &got) == cdc::kPackSizesCheck);
    h = good, h.data_bytes = 65;
    CHECK(cdc::pack_check_header(h, l.total, &got) == cdc::kPackSizesCheck);
    h = good, h.n_spans = 1ull << 59, h.n_chunks = 0;
    CHECK(cdc::pack_check_header(h, ~0ull, &got) == cdc::kPackSizesCheck);
    h = good, h.n_spans = 6;
    CHECK(cdc::pack_check_header(h, ~0ull, &got) == cdc::kPackTotalCheck);
    h = good, h.n_chunks = 4;
    CHECK(cdc::pack_check_header(h, ~0ull, &got) == cdc::kPackTotalCheck);
    h = good, h.total_bytes += 1;
    CHECK(cdc::pack_check_header(h, ~0ull, &got) == cdc::kPackTotalCheck);
    const unsigned char magic[8] = {'C', 'D', 'C', 'P', 'A', 'C', 'K', '1'};
    uint64_t m = 0;
    std::memcpy(&m, magic, 8);
    CHECK(m == cdc::kPackMagic);  // this program runs on a little-endian host, as the format is
    for (uint32_t c = 1; c < cdc::kPackChecks; ++c) CHECK(std::strcmp(cdc::pack_check_name(c), "ok") != 0);
}

// The index sections as heap arrays of exactly their entries.
struct Sections {
    uint64_t n, nc;
    uint8_t *digest;
    uint64_t *length, *span_chunk, *chunk_span, *chunk_off;
    uint64_t data_bytes, file_size, external;

    Sections(uint64_t n_, uint64_t nc_) : n(n_), nc(nc_) {
        digest = static_cast<uint8_t *>(std::malloc(n * 32 + 1));
        length = static_cast<uint64_t *>(std::malloc(n * 8 + 1));
        span_chunk = static_cast<uint64_t *>(std::malloc(n * 8 + 1));
        chunk_span = static_cast<uint64_t *>(std::malloc(nc * 8 + 1));
        chunk_off = static_cast<uint64_t *>(std::malloc((nc + 1) * 8));
        data_bytes = file_size = external = 0;
    }
    ~Sections() {
        std::free(digest), std::free(length), std::free(span_chunk), std::free(chunk_span), std::free(chunk_off);
    }
    cdc::PackView view() const {
        cdc::PackView v;
        v.digest = digest, v.length = length, v.span_chunk = span_chunk, v.chunk_span = chunk_span;
        v.chunk_off = chunk_off, v.n_spans = n, v.n_chunks = nc;
        v.data_bytes = data_bytes, v.file_size = file_size, v.external_spans = external;
        return v;
    }
};

// A valid pack's sections: n spans over nc distinct carried chunks plus some externals.
Sections *make_good(uint64_t n, uint64_t nc) {
    Sections *s = new Sections(n, nc);
    std::vector<uint64_t> ident(n);  // which content a span has: < nc carried, >= nc external
    uint64_t next = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t left = n - i, need = nc - next;
        if (need == left || (need && rnd() % 2)) ident[i] = next++;
        else if (next && rnd() % 2) ident[i] = rnd() % next;
        else ident[i] = nc + rnd() % 3;
    }
    std::vector<uint64_t> len_of(nc + 3);
    for (auto &l : len_of) l = rnd() % 4 == 0 ? 0 : rnd() % 70;
    uint64_t at = 0;
    for (uint64_t i = 0, k = 0; i < n; ++i) {
        const uint64_t id = ident[i];
        for (int b = 0; b < 32; ++b) s->digest[32 * i + b] = (uint8_t)(id * 37 + b);
        s->length[i] = len_of[id];
        s->file_size += len_of[id];
        if (id < nc) {
            s->span_chunk[i] = id;
            if (id == k) {
                s->chunk_span[k] = i;
                s->chunk_off[k] = at;
                at += (len_of[id] + 15) & ~15ull;
                ++k;
            }
        } else {
            s->span_chunk[i] = cdc::kPackExternal;
            ++s->external;
        }
    }
    s->chunk_off[nc] = at;
    s->data_bytes = at;
    return s;
}

// Every predicate by brute force, with 128-bit arithmetic and explicit bounds.
struct Verdict {
    bool ok[cdc::kPackChecks];
};
Verdict brute(const Sections &s) {
    Verdict v;
    for (auto &o : v.ok) o = true;
    const uint64_t n = s.n, nc = s.nc;
    for (uint64_t k = 0; k < nc; ++k) {
        const uint64_t i = s.chunk_span[k];
        if (i >= n || (k > 0 && s.chunk_span[k - 1] >= i)) v.ok[cdc::kPackChunkSpanCheck] = false;
        if (i < n && s.span_chunk[i] != k) v.ok[cdc::kPackBackrefCheck] = false;
        if (k == 0 && s.chunk_off[0] != 0) v.ok[cdc::kPackChunkOffCheck] = false;
        if (i < n && (u128)s.chunk_off[k] + pad(s.length[i]) != (u128)s.chunk_off[k + 1])
            v.ok[cdc::kPackChunkOffCheck] = false;
    }
    u128 sum = 0;
    uint64_t ext = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t c = s.span_chunk[i];
        sum += s.length[i];
        if (c == cdc::kPackExternal) {
            ++ext;
            continue;
        }
        if (c >= nc) {
            v.ok[cdc::kPackSpanChunkCheck] = false;
            continue;
        }
        const uint64_t j = s.chunk_span[c];
        if (j < n && (s.length[i] != s.length[j] || std::memcmp(s.digest + 32 * i, s.digest + 32 * j, 32) != 0))
            v.ok[cdc::kPackSameCheck] = false;
    }
    if (n && (s.chunk_off[nc] != s.data_bytes || (nc == 0 && s.chunk_off[0] != 0))) v.ok[cdc::kPackDataBytesCheck] = false;
    if (sum != (u128)s.file_size) v.ok[cdc::kPackFileSizeCheck] = false;
    if (ext != s.external) v.ok[cdc::kPackExternalCheck] = false;
    return v;
}

// The predicates as the validation kernel runs them: one index at a time.
Verdict plan(const Sections &s) {
    Verdict v;
    for (auto &o : v.ok) o = true;
    const cdc::PackView p = s.view();
    for (uint64_t k = 0; k < s.nc; ++k) {
        if (!cdc::pack_ok_chunk_span(p, k)) v.ok[cdc::kPackChunkSpanCheck] = false;
        if (!cdc::pack_ok_backref(p, k)) v.ok[cdc::kPackBackrefCheck] = false;
        if (!cdc::pack_ok_chunk_off(p, k)) v.ok[cdc::kPackChunkOffCheck] = false;
    }
    cdc::PackSum sum{0, 0};
    uint64_t ext = 0;
    for (uint64_t i = 0; i < s.n; ++i) {
        if (!cdc::pack_ok_span_chunk(p, i)) v.ok[cdc::kPackSpanChunkCheck] = false;
        if (!cdc::pack_ok_same(p, i)) v.ok[cdc::kPackSameCheck] = false;
        sum = cdc::pack_sum_add(sum, cdc::PackSum{s.length[i], 0});
        ext += s.span_chunk[i] == cdc::kPackExternal;
    }
    if (!cdc::pack_ok_data_bytes(p)) v.ok[cdc::kPackDataBytesCheck] = false;
    if (!cdc::pack_ok_file_size(p, sum)) v.ok[cdc::kPackFileSizeCheck] = false;
    if (ext != s.external) v.ok[cdc::kPackExternalCheck] = false;
    return v;
}

bool all_ok(const Verdict &v) {
    for (bool o : v.ok)
        if (!o) return false;
    return true;
}

void compare(const Sections &s, int line) {
    const Verdict a = brute(s), b = plan(s);
    for (uint32_t c = 0; c < cdc::kPackChecks; ++c)
        if (a.ok[c] != b.ok[c]) {
            std::fprintf(stderr, "line %d: check '%s': brute force %d, plan %d\n", line, cdc::pack_check_name(c),
                         (int)a.ok[c], (int)b.ok[c]);
            ++failures;
        }
}

uint64_t wild() {
    switch (rnd() % 6) {
        case 0: return ~0ull;
        case 1: return ~0ull - rnd() % 40;
        case 2: return rnd();
        case 3: return 1ull << (rnd() % 64);
        default: return rnd() % 80;
    }
}

void check_predicates() {
    // A pack without spans has no section to check.
    {
        Sections *s = make_good(0, 0);
        CHECK(all_ok(plan(*s)) && all_ok(brute(*s)));
        delete s;
    }
    for (int t = 0; t < 3000; ++t) {
        const uint64_t n = t < 40 ? (uint64_t)t % 8 : rnd() % 40, nc = n ? rnd() % (n + 1) : 0;
        Sections *s = make_good(n, nc);
        const Verdict good = plan(*s);
        CHECK(all_ok(good));
        CHECK(all_ok(brute(*s)));
        // One edit: any entry of any section, or a header field, to a wild value.
        for (int e = 0; e < 30; ++e) {
            uint64_t *slot = nullptr;
            switch (rnd() % 8) {
                case 0: slot = n ? &s->length[rnd() % n] : nullptr; break;
                case 1: slot = n ? &s->span_chunk[rnd() % n] : nullptr; break;
                case 2: slot = nc ? &s->chunk_span[rnd() % nc] : nullptr; break;
                case 3: slot = &s->chunk_off[rnd() % (nc + 1)]; break;
                case 4: slot = &s->data_bytes; break;
                case 5: slot = &s->file_size; break;
                case 6: slot = &s->external; break;
                default: slot = n ? reinterpret_cast<uint64_t *>(s->digest + 32 * (rnd() % n)) : nullptr; break;
            }
            if (!slot) continue;
            uint64_t old;
            std::memcpy(&old, slot, 8);
            const uint64_t v = rnd() % 3 == 0 ? old + 1 : (rnd() % 3 == 0 ? old + 16 : wild());
            std::memcpy(slot, &v, 8);
            compare(*s, __LINE__);
            if (rnd() % 4) std::memcpy(slot, &old, 8);  // sometimes the edits pile up
            else if (all_ok(plan(*s)) != all_ok(brute(*s))) ++failures;
        }
        delete s;
    }
    // The length sum wraps 2^64 exactly onto file_size: refused, not wrapped.
    {
        Sections s(2, 0);
        s.length[0] = 1ull << 63, s.length[1] = (1ull << 63) + 5;
        s.span_chunk[0] = s.span_chunk[1] = cdc::kPackExternal;
        s.chunk_off[0] = 0;
        s.external = 2, s.file_size = 5;
        const Verdict v = plan(s);
        CHECK(!v.ok[cdc::kPackFileSizeCheck] && !brute(s).ok[cdc::kPackFileSizeCheck]);
        s.file_size = (1ull << 63) + 5, s.length[0] = 0;
        CHECK(plan(s).ok[cdc::kPackFileSizeCheck]);
    }
    // chunk_off steps that wrap: a decreasing pair whose difference wraps to the padded length.
    {
        Sections s(1, 1);
        s.length[0] = 32, s.span_chunk[0] = 0, s.chunk_span[0] = 0;
        s.chunk_off[0] = 0, s.chunk_off[1] = 32;
        s.data_bytes = 32, s.file_size = 32;
        std::memset(s.digest, 7, 32);
        CHECK(all_ok(plan(s)));
        s.length[0] = ~0ull - 3;  // round_up passes 2^64
        CHECK(!plan(s).ok[cdc::kPackChunkOffCheck] && !brute(s).ok[cdc::kPackChunkOffCheck]);
        s.length[0] = ~0ull - 15, s.chunk_off[0] = 16, s.chunk_off[1] = 0;  // 0 - 16 wraps to the padded length
        CHECK(!plan(s).ok[cdc::kPackChunkOffCheck] && !brute(s).ok[cdc::kPackChunkOffCheck]);
    }
}

}  // namespace

int main() {
    check_layout();
    check_header();
    check_predicates();
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::printf("pack plan ok\n");
    return 0;
}
