// read_plan_check.cpp -- the arithmetic of the file layer's range planner
// (chunkfs_amd/csrc/read_plan.hpp) against brute force, as a plain C++ program
// for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I chunkfs_amd/csrc tools/read_plan_check.cpp -o read_plan_check && ./read_plan_check
// The host sizes grids and scratch from read_bound before a request is
// resolved on the device; a bound below what read_resolve then yields would
// drop pieces.  For seeded tables and requests of all three kinds it checks
// that the resolved span count and the tiles of the resolved pieces stay inside
// the bounds, that each kind resolves to what its definition says, and that the
// bounds equal the two loops they were taken from, written out again below.
// Every offset table is a heap array of its exact size, so a search that steps
// outside one is an error the sanitizer reports.  Exit code 0 and "read plan
// ok" on success.
#include <cstdio>
#include <vector>

#include "read_plan.hpp"

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

// A file as the host knows it: the table, and what it keeps of the append's statistics.
struct File {
    std::vector<uint64_t> off;  // n + 1
    uint64_t n = 0, size = 0, min_len = ~0ull, zeros = 0;
};

File make_file(uint64_t n, const uint64_t *lengths, uint64_t n_lengths) {
    File f;
    f.n = n;
    f.off.push_back(0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = lengths[rnd() % n_lengths];
        f.off.push_back(f.off.back() + len);
        if (len == 0) ++f.zeros;
        else if (len < f.min_len) f.min_len = len;
    }
    f.size = f.off.back();
    return f;
}

// 0 .. limit + 2, and now and then the largest value: the sums must not wrap.
uint64_t draw(uint64_t limit) { return rnd() % 16 == 0 ? ~0ull : rnd() % (limit + 3); }

// ---- the bounds as the two read paths computed them before they shared read_bound --
uint64_t old_spans_bound(const File &f, uint64_t bytes) {
    const uint64_t fit = f.min_len == ~0ull ? 0 : bytes / f.min_len;
    const uint64_t bound = f.zeros + fit + 2;
    return bound < f.n ? bound : f.n;
}
void old_unscrubbed(const File &f, uint32_t kind, uint64_t b, uint64_t cap, uint64_t *max_pieces, uint64_t *max_tiles) {
    uint64_t bytes = f.size < cap ? f.size : cap;
    if (kind != cdc::kReadComplete && b < bytes) bytes = b;
    const uint64_t spans = kind == cdc::kReadComplete ? f.n : old_spans_bound(f, bytes);
    *max_pieces += spans;
    if (bytes) *max_tiles += bytes / cdc::kReadTile + 2 * spans;
}
void old_scrubbed(const File &f, uint32_t kind, uint64_t b, uint64_t cap, uint64_t *max_spans, uint64_t *max_bytes) {
    uint64_t bytes = f.size < cap ? f.size : cap;
    if (kind != cdc::kReadComplete && b < bytes) bytes = b;
    *max_spans += kind == cdc::kReadComplete ? f.n : old_spans_bound(f, bytes);
    *max_bytes += bytes;
}

// ---- the three kinds by their definitions, one span at a time ------------------------
cdc::ReadSpans by_definition(const File &f, uint32_t kind, uint64_t a, uint64_t b) {
    cdc::ReadSpans r{0, 0, 0, 0};
    if (f.n == 0) return r;
    if (kind == cdc::kReadComplete) {  // every span
        r.hi = f.size;
        r.count = f.n;
    } else if (kind == cdc::kReadSegment) {  // skip_while(offset < cursor), take_while(running total <= seg)
        uint64_t i = 0;
        while (i < f.n && f.off[i] < a) ++i;
        if (i == f.n) return r;
        r.first = i;
        r.lo = r.hi = f.off[i];
        for (; i < f.n; ++i) {
            const uint64_t len = f.off[i + 1] - f.off[i];
            if (len > b || r.hi - r.lo > b - len) break;
            r.hi += len;
            ++r.count;
        }
    } else {  // the bytes [a, a + b) clipped to the file, from the span of the first to the span of the last
        r.lo = a < f.size ? a : f.size;
        r.hi = b > f.size - r.lo ? f.size : r.lo + b;
        if (r.hi == r.lo) return r;
        uint64_t i = 0, j = 0;
        while (!(f.off[i] <= r.lo && r.lo < f.off[i + 1])) ++i;
        while (!(f.off[j] <= r.hi - 1 && r.hi - 1 < f.off[j + 1])) ++j;
        r.first = i;
        r.count = j - i + 1;
    }
    return r;
}

void check_request(const File &f, uint32_t kind, uint64_t a, uint64_t b, uint64_t cap, uint64_t dst) {
    const cdc::ReadSpans r = cdc::read_resolve(f.off.data(), f.n, kind, a, b, cap);
    const cdc::ReadBound bd = cdc::read_bound(kind, b, cap, f.n, f.size, f.min_len, f.zeros);

    // The kind's definition; a destination that is too small takes nothing and learns the size.
    const cdc::ReadSpans want = by_definition(f, kind, a, b);
    CHECK(r.lo == want.lo && r.hi == want.hi && r.first == want.first);
    CHECK(r.count == (want.hi - want.lo > cap ? 0 : want.count));
    CHECK(r.lo <= r.hi && r.hi <= f.size && r.first + r.count <= f.n);
    if (kind == cdc::kReadSegment) CHECK(r.hi - r.lo <= b);
    if (kind == cdc::kReadRange && a <= f.size) CHECK(r.lo == a && r.hi - r.lo == (b < f.size - a ? b : f.size - a));

    // The pieces as pieces_kernel cuts them: only the first and the last are trimmed.
    uint64_t bytes = 0, tiles = 0;
    for (uint64_t k = 0; k < r.count; ++k) {
        const uint64_t s0 = f.off[r.first + k], s1 = f.off[r.first + k + 1];
        const uint64_t from = s0 > r.lo ? s0 : r.lo, to = s1 < r.hi ? s1 : r.hi;
        const uint64_t len = to > from ? to - from : 0;
        const uint64_t at = dst + (from - r.lo);
        CHECK(len == 0 || from - r.lo == bytes);  // back to back in the destination
        bytes += len;
        tiles += len ? ((at & (cdc::kReadAlign - 1)) + len + (cdc::kReadTile - 1)) / cdc::kReadTile : 0;
    }
    if (r.count) CHECK(bytes == r.hi - r.lo);

    // The bounds hold ...
    CHECK(r.count <= bd.spans);
    CHECK(bytes <= bd.bytes);
    CHECK(tiles <= (bd.bytes ? cdc::read_tiles_bound(bd.bytes, bd.spans) : 0));
    // ... and are the ones both read paths had.
    uint64_t pieces = 0, otiles = 0, spans = 0, obytes = 0;
    old_unscrubbed(f, kind, b, cap, &pieces, &otiles);
    old_scrubbed(f, kind, b, cap, &spans, &obytes);
    CHECK(bd.spans == pieces && bd.spans == spans && bd.bytes == obytes);
    CHECK((bd.bytes ? cdc::read_tiles_bound(bd.bytes, bd.spans) : 0) == otiles);
    CHECK(cdc::spans_bound(f.n, f.min_len, f.zeros, bd.bytes) == old_spans_bound(f, bd.bytes));
}

void check_file(const File &f, int requests) {
    for (int q = 0; q < requests; ++q)
        check_request(f, (uint32_t)(rnd() % 3), draw(f.size), draw(f.size), draw(f.size), rnd() % (4 * cdc::kReadTile));
}

}  // namespace

int main() {
    // A file without spans resolves to nothing, whatever is asked.
    check_file(make_file(0, nullptr, 1), 64);
    // Short tables, half of the lengths 0 in places: equal offsets, ends on boundaries, ranges inside one span.
    const uint64_t small[] = {0, 0, 1, 2, 3, 5, 8};
    for (int t = 0; t < 12000; ++t) check_file(make_file(1 + rnd() % 12, small, 7), 16);
    // Only empty spans: a file of n spans and no byte.
    const uint64_t none[] = {0};
    for (uint64_t n = 1; n <= 4; ++n) check_file(make_file(n, none, 1), 64);
    // Long tables with spans around the tile size: whole tiles, and pieces that straddle them.
    const uint64_t T = cdc::kReadTile;
    const uint64_t tiled[] = {0, 1, 15, 16, 17, T - 16, T - 1, T, T + 1, 2 * T, 3 * T + 5};
    for (int t = 0; t < 150; ++t) check_file(make_file(65 + rnd() % 200, tiled, 11), 64);
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::printf("read plan ok\n");
    return 0;
}
