// splice_plan_check.cpp -- the index arithmetic of cdc_file_splice_device
// (chunkfs_amd/csrc/splice_plan.hpp) against brute force, as a plain C++ program
// for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I chunkfs_amd/csrc tools/splice_plan_check.cpp -o splice_plan_check && ./splice_plan_check
// Every table is a heap array of exactly n + 1 entries, so a search that steps
// outside it is an error the sanitizer reports.  Exit code 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "splice_plan.hpp"

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

// off[0 .. n] with off[0] = 0: span lengths 0 .. 20, many of them 0.
uint64_t *make_table(uint64_t n) {
    uint64_t *off = static_cast<uint64_t *>(std::malloc((n + 1) * sizeof(uint64_t)));
    off[0] = 0;
    for (uint64_t i = 0; i < n; ++i) off[i + 1] = off[i] + (rnd() % 3 == 0 ? 0 : rnd() % 21);
    return off;
}

void check_tables() {
    for (int t = 0; t < 400; ++t) {
        const uint64_t n = t < 20 ? (uint64_t)t : rnd() % 70;
        uint64_t *off = make_table(n);
        const uint64_t size = off[n];
        for (uint64_t offset = 0; offset <= size; ++offset) {
            uint64_t want = 0;
            for (uint64_t i = 0; i < n; ++i)
                if (off[i] + cdc::kSpliceBack <= offset) want = i;
            CHECK(cdc::splice_start_span(off, n, offset) == want);
        }
        for (uint64_t x = 0; x <= size + 3; ++x) {  // e - insert_len + remove_len = x, three ways
            uint64_t want = n + 1;
            for (uint64_t j = 0; j <= n; ++j)
                if (off[j] == x) {
                    want = j;
                    break;
                }
            if (n == 0) want = x == 0 ? 0 : 1;
            const uint64_t forms[3][3] = {{x, 0, 0}, {x + 5, 0, 5}, {0, x, 0}};
            for (const auto &f : forms) {
                if (f[0] < f[2]) continue;
                uint64_t j = ~0ull;
                const bool hit = cdc::splice_old_boundary(off, n, f[0], f[1], f[2], &j);
                CHECK(hit == (want <= n));
                if (hit) CHECK(j == want);
            }
        }
        std::free(off);
    }
    uint64_t j = 7;
    CHECK(cdc::splice_start_span(nullptr, 0, 12345) == 0);
    CHECK(cdc::splice_old_boundary(nullptr, 0, 10, 0, 10, &j) && j == 0);
    CHECK(!cdc::splice_old_boundary(nullptr, 0, 11, 0, 10, &j));
}

void check_ranges() {
    const uint64_t top = ~0ull;
    CHECK(cdc::splice_range_ok(100, 0, 100) && cdc::splice_range_ok(100, 100, 0) && cdc::splice_range_ok(0, 0, 0));
    CHECK(!cdc::splice_range_ok(100, 101, 0) && !cdc::splice_range_ok(100, 50, 51));
    CHECK(!cdc::splice_range_ok(100, 1, top) && !cdc::splice_range_ok(100, top, 1) && !cdc::splice_range_ok(top, top, 1));
    uint64_t after = 0;
    CHECK(cdc::splice_size_after(100, 40, 7, &after) && after == 67);
    CHECK(cdc::splice_size_after(top, top, top, &after) && after == top);
    CHECK(!cdc::splice_size_after(top, 0, 1, &after) && !cdc::splice_size_after(top - 5, 2, 8, &after));
    CHECK(cdc::splice_sat_add(top, 1) == top && cdc::splice_sat_add(top - 1, 1) == top && cdc::splice_sat_add(3, 4) == 7);
    CHECK(cdc::splice_sat_mul(top / 2, 3) == top && cdc::splice_sat_mul(0, top) == 0 && cdc::splice_sat_mul(top, 0) == 0);
    CHECK(cdc::splice_sat_mul(1ull << 62, 4) == top && cdc::splice_sat_mul(1ull << 61, 4) == 1ull << 63);
}

void check_windows() {
    // The schedule of the header: 4 max + 8, 16 max + 8, ... past the inserted bytes, clipped to the file.
    CHECK(cdc::splice_window_end(1000000000, 1000, 10, 1024, 1) == 1010 + 4096 + 8);
    CHECK(cdc::splice_window_end(1000000000, 1000, 10, 1024, 2) == 1010 + 16384 + 8);
    CHECK(cdc::splice_window_end(1000000000, 1000, 10, 1024, 3) == 1010 + 65536 + 8);
    CHECK(cdc::splice_window_end(2000, 1000, 10, 1024, 1) == 2000);
    CHECK(cdc::splice_window_end(0, 0, 0, 512, 1) == 0);
    const uint64_t top = ~0ull;
    for (uint32_t round = 1; round < 200; ++round) {  // no wrap however far the rounds go
        CHECK(cdc::splice_window_end(top, top - 100, 50, 1u << 24, round) >= top - 50);
        CHECK(cdc::splice_window_end(top, 5, top - 10, 1, round) == top);
        const uint64_t a = cdc::splice_window_end(1ull << 60, 123, 456, 4096, round);
        const uint64_t b = cdc::splice_window_end(1ull << 60, 123, 456, 4096, round + 1);
        CHECK(a <= b && b <= 1ull << 60);  // the windows only grow, and end with the file
    }
    CHECK(cdc::splice_window_end(1ull << 60, 123, 456, 4096, 40) == 1ull << 60);
    // Trust: everything a chunk can read lies inside the window, or the window ends the file.
    CHECK(cdc::splice_trusted(0, 1024, 1032, 5000) && !cdc::splice_trusted(1, 1024, 1032, 5000));
    CHECK(cdc::splice_trusted(4999, 1024, 5000, 5000) && !cdc::splice_trusted(4999, 1024, 5000, 5001));
    CHECK(!cdc::splice_trusted(top - 3, 1024, top - 1, top) && cdc::splice_trusted(top - 3, 1024, top, top));
    // A round whose window ends with the file trusts every chunk, so the rounds end.
    for (int t = 0; t < 2000; ++t) {
        const uint64_t size_after = rnd() % 100000, maxc = 1 + rnd() % 2000;
        const uint64_t offset = size_after ? rnd() % (size_after + 1) : 0;
        const uint64_t insert_len = rnd() % (size_after - offset + 1);
        uint32_t round = 1;
        uint64_t prev = 0;
        for (;; ++round) {
            const uint64_t end_w = cdc::splice_window_end(size_after, offset, insert_len, maxc, round);
            CHECK(end_w >= prev && end_w <= size_after && end_w >= (offset + insert_len < size_after ? offset + insert_len : size_after));
            prev = end_w;
            if (end_w == size_after) break;
            CHECK(round < 40);
            if (round >= 40) break;
        }
        CHECK(cdc::splice_trusted(rnd() % (size_after + 1), maxc, prev, size_after));
    }
}

}  // namespace

int main() {
    check_tables();
    check_ranges();
    check_windows();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::puts("splice plan ok");
    return 0;
}
