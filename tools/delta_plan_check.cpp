// delta_plan_check.cpp -- chunkfs_amd/csrc/delta_plan.hpp against brute force, as
// a plain C++ program for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I chunkfs_amd/csrc tools/delta_plan_check.cpp
// It walks the stages of delta.hip on the host over random tables: the sorted
// pairs and the nearest-offset search with its tie rule; the runs; per region
// every tile and every lane's segment of either direction, which must cover the
// bytes the search may read exactly once and never leave either file; the clip;
// and the head flags, whose ops must be the canonical form of the plain list.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "delta_plan.hpp"

using namespace cdc;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

struct Table {
    std::vector<uint64_t> off;   // n + 1
    std::vector<uint32_t> slot;  // n
    std::vector<uint8_t> bytes;
    uint64_t n() const { return slot.size(); }
    uint64_t size() const { return off.back(); }
};

struct Op {
    uint64_t b_off, len;
    bool copy;
    int64_t d;
    bool operator==(const Op &o) const { return b_off == o.b_off && len == o.len && copy == o.copy && (!copy || d == o.d); }
};

// Blocks over a two-letter alphabet, so that edges match by accident too; block 0 is empty.
std::vector<std::vector<uint8_t>> make_blocks(uint32_t count, uint32_t max_len) {
    std::vector<std::vector<uint8_t>> b(count);
    for (uint32_t i = 1; i < count; ++i) {
        b[i].resize(1 + rnd() % max_len);
        for (auto &x : b[i]) x = (uint8_t)(rnd() % 2);
    }
    return b;
}

Table make_table(const std::vector<std::vector<uint8_t>> &blocks, uint32_t spans) {
    Table t;
    t.off.push_back(0);
    for (uint32_t i = 0; i < spans; ++i) {
        const uint32_t s = (uint32_t)(rnd() % blocks.size());
        t.slot.push_back(s);
        t.bytes.insert(t.bytes.end(), blocks[s].begin(), blocks[s].end());
        t.off.push_back(t.bytes.size());
    }
    return t;
}

void check_pair(const Table &a, const Table &b, uint64_t *regions_seen, uint64_t *tiles_seen) {
    const uint64_t na = a.n(), nb = b.n(), size_a = a.size(), size_b = b.size();
    if (!size_a || !size_b) return;  // no device pass
    // 1. the sorted pairs: stable, so each group ascends in span index and in offset
    std::vector<uint32_t> idx(na);
    for (uint32_t i = 0; i < na; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return a.slot[x] < a.slot[y]; });
    std::vector<uint64_t> key(na);
    for (uint64_t p = 0; p < na; ++p) key[p] = a.slot[idx[p]];
    // 2. anchors against a scan of all of A
    std::vector<int64_t> diag(nb);
    for (uint64_t j = 0; j < nb; ++j) {
        if (b.off[j + 1] == b.off[j]) {
            diag[j] = kDeltaSkip;
            continue;
        }
        uint64_t g0, g1;
        delta_group(key.data(), na, b.slot[j], &g0, &g1);
        int64_t want = kDeltaNone;
        uint64_t best = ~0ull, best_off = 0;
        for (uint64_t i = 0; i < na; ++i) {
            if (a.slot[i] != b.slot[j]) continue;
            const uint64_t dist = a.off[i] > b.off[j] ? a.off[i] - b.off[j] : b.off[j] - a.off[i];
            if (dist < best || (dist == best && a.off[i] < best_off)) best = dist, best_off = a.off[i];
        }
        if (best != ~0ull) want = delta_diagonal(best_off, b.off[j]);
        diag[j] = g0 < g1 ? delta_diagonal(a.off[delta_nearest(a.off.data(), idx.data(), g0, g1, b.off[j])], b.off[j])
                          : kDeltaNone;
        CHECK(diag[j] == want);
        CHECK((g0 < g1) == (best != ~0ull));
    }
    // 3. runs, as the flag kernel finds them
    std::vector<uint64_t> rb;
    std::vector<int64_t> rd;
    for (uint64_t j = 0; j < nb; ++j) {
        if (diag[j] == kDeltaSkip) continue;
        const bool head = b.off[j] == 0 || diag[diff_span_at(b.off.data(), nb, b.off[j] - 1)] != diag[j];
        CHECK(head == (rd.empty() || rd.back() != diag[j]));
        if (head) rb.push_back(b.off[j]), rd.push_back(diag[j]);
    }
    const uint64_t n_runs = rb.size();
    rb.push_back(size_b);
    // 4. edges per region, tile by tile and lane by lane; 5. heads
    std::vector<Op> plain, got;
    std::vector<uint64_t> es(n_runs, 0), fs(n_runs, 0);
    auto region_of = [&](uint64_t k) {
        DeltaRegion g;
        g.l = rb[k], g.r = rb[k + 1];
        g.dl = k ? rd[k - 1] : 0;
        g.dr = k + 1 < n_runs ? rd[k + 1] : (int64_t)(size_a - size_b);
        return g;
    };
    for (uint64_t k = 0; k < n_runs; ++k) {
        const DeltaRegion g = region_of(k);
        const uint64_t len = g.r - g.l;
        if (rd[k] != kDeltaNone) {
            plain.push_back({g.l, len, true, rd[k]});
            continue;
        }
        ++*regions_seen;
        CHECK(k == 0 || rd[k - 1] != kDeltaNone);
        const uint64_t cap = delta_fwd_cap(g, size_a), floor = delta_bwd_floor(g, size_a);
        CHECK(cap <= len && floor >= g.l && floor <= g.r);
        uint64_t fwd = cap, bwd = floor;
        std::vector<uint8_t> seen_f(len, 0), seen_b(len, 0);
        for (uint64_t t = 0; t < delta_tiles(len); ++t) {
            ++*tiles_seen;
            for (int dir = 0; dir < 2; ++dir) {
                uint64_t x0, x1;
                if (dir == 0) delta_fwd_tile(g, t, &x0, &x1);
                else delta_bwd_tile(g, t, &x0, &x1);
                CHECK(g.l <= x0 && x0 < x1 && x1 <= g.r && x1 - x0 <= kDeltaTile);
                for (uint32_t lane = 0; lane < kDeltaTile / kDeltaSeg; ++lane) {
                    uint64_t s0, s1;
                    const bool any = dir == 0 ? delta_segment(x0, x1, lane, false, g.l, g.l + cap, &s0, &s1)
                                              : delta_segment(x0, x1, lane, true, floor, g.r, &s0, &s1);
                    if (!any) continue;
                    CHECK(x0 <= s0 && s0 < s1 && s1 <= x1 && s1 - s0 <= kDeltaSeg);
                    for (uint64_t x = s0; x < s1; ++x) {
                        const uint64_t y = delta_a_index(x, dir == 0 ? g.dl : g.dr);
                        CHECK(y < size_a);  // vectors: ASan sees an index out of either file
                        ++(dir == 0 ? seen_f : seen_b)[x - g.l];
                        if (b.bytes[x] == a.bytes[y]) continue;
                        if (dir == 0 && x - g.l < fwd) fwd = x - g.l;
                        if (dir == 1 && x + 1 > bwd) bwd = x + 1;
                    }
                }
            }
        }
        for (uint64_t i = 0; i < len; ++i) {
            CHECK(seen_f[i] == (i < cap ? 1 : 0));
            CHECK(seen_b[i] == (g.l + i >= floor ? 1 : 0));
        }
        uint64_t e = 0, f = 0;  // the rule, byte by byte
        auto inside = [&](int64_t y) { return y >= 0 && (uint64_t)y < size_a; };
        while (e < len && inside((int64_t)(g.l + e) + g.dl) && b.bytes[g.l + e] == a.bytes[g.l + e + g.dl]) ++e;
        while (f < len - e && inside((int64_t)(g.r - 1 - f) + g.dr) && b.bytes[g.r - 1 - f] == a.bytes[g.r - 1 - f + g.dr])
            ++f;
        CHECK(fwd == e);
        CHECK(delta_clip(len, fwd, g.r - bwd) == f);
        es[k] = e, fs[k] = f;
        plain.push_back({g.l, e, true, g.dl});
        plain.push_back({g.l + e, len - e - f, false, 0});
        plain.push_back({g.r - f, f, true, g.dr});
    }
    std::vector<Op> want;  // canonical form of the plain list
    for (const Op &o : plain) {
        if (!o.len) continue;
        if (!want.empty() && delta_merges(want.back().copy, want.back().d, o.copy, o.d)) want.back().len += o.len;
        else want.push_back(o);
    }
    for (uint64_t k = 0; k < n_runs; ++k) {  // as the head kernel writes them: b_off and kind
        const DeltaRegion g = region_of(k);
        if (rd[k] == kDeltaNone) {
            const uint32_t h = delta_region_heads(g.r - g.l, es[k], fs[k], g.dl, g.dr, k > 0);
            if (h & 1) got.push_back({g.l, 0, true, g.dl});
            if (h & 2) got.push_back({g.l + es[k], 0, false, 0});
            if (h & 4) got.push_back({g.r - fs[k], 0, true, g.dr});
        } else {
            bool h = true;
            if (k && rd[k - 1] == kDeltaNone) {
                const DeltaRegion p = region_of(k - 1);
                h = delta_copy_head_after_region(p.r - p.l, es[k - 1], fs[k - 1], p.dl, rd[k]);
            }
            if (h) got.push_back({g.l, 0, true, rd[k]});
        }
    }
    for (size_t i = 0; i < got.size(); ++i) got[i].len = (i + 1 < got.size() ? got[i + 1].b_off : size_b) - got[i].b_off;
    CHECK(got.size() == want.size());
    for (size_t i = 0; i < got.size(); ++i) CHECK(got[i] == want[i]);
    CHECK(got.size() <= 3 * nb);
}

}  // namespace

int main() {
    uint64_t regions = 0, tiles = 0, pairs = 0;
    // the tie rule, by hand: equal distances take the smaller offset; the ends of a group
    {
        const uint64_t off_a[] = {0, 10, 20, 30, 40};
        const uint32_t idx[] = {0, 2, 3};
        CHECK(delta_nearest(off_a, idx, 0, 3, 10) == 0);  // 0 and 20 tie
        CHECK(delta_nearest(off_a, idx, 0, 3, 11) == 2 && delta_nearest(off_a, idx, 0, 3, 9) == 0);
        CHECK(delta_nearest(off_a, idx, 0, 3, 25) == 2 && delta_nearest(off_a, idx, 0, 3, 26) == 3);
        CHECK(delta_nearest(off_a, idx, 0, 3, 1000) == 3 && delta_nearest(off_a, idx, 1, 2, 0) == 2);
        CHECK(delta_clip(10, 4, 9) == 6 && delta_clip(10, 10, 3) == 0 && delta_clip(10, 0, 3) == 3);
    }
    for (int round = 0; round < 400; ++round) {
        const auto blocks = make_blocks(2 + (uint32_t)(rnd() % 6), round % 8 == 0 ? 9000 : 1 + (uint32_t)(rnd() % 40));
        const Table a = make_table(blocks, (uint32_t)(rnd() % 14)), b = make_table(blocks, (uint32_t)(rnd() % 14));
        check_pair(a, b, &regions, &tiles);
        // and against tables that share no slot: the prefix and suffix rule
        Table c = make_table(blocks, 1 + (uint32_t)(rnd() % 5));
        for (auto &s : c.slot) s += 100;
        check_pair(a, c, &regions, &tiles);
        check_pair(c, b, &regions, &tiles);
        pairs += 3;
    }
    CHECK(regions > 200 && tiles > regions);
    std::printf("delta plan ok: %llu pairs, %llu regions, %llu tiles\n", (unsigned long long)pairs,
                (unsigned long long)regions, (unsigned long long)tiles);
    return 0;
}
