// diff_plan_check.cpp -- the index arithmetic of cdc_files_diff_device
// (chunkfs_amd/csrc/diff_plan.hpp) against brute force, as a plain C++ program
// for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I chunkfs_amd/csrc tools/diff_plan_check.cpp -o diff_plan_check && ./diff_plan_check
// It walks the device path's stages on the host with the header's functions:
// the candidates' flags and their scan, the ranks, the sharing rule, the tiles
// of the compared pieces with their masks, the per-tile run starts and their
// scan, the emit with its carries and the tail.  Every array is a heap array of
// its exact size, so a step outside one is an error the sanitizer reports.
// Exit code 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "diff_plan.hpp"

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

typedef std::vector<std::pair<uint64_t, uint64_t>> Ranges;

struct Table {
    std::vector<uint64_t> off;    // n + 1
    std::vector<uint32_t> slot;   // n
    uint64_t n() const { return slot.size(); }
    uint64_t size() const { return off.back(); }
};

// Span lengths 0 .. maxlen, a third of them 0; slots from a small set, so that
// two tables often name one slot at one offset -- and at different ones.
Table make_table(uint64_t n, uint64_t maxlen) {
    Table t;
    t.off.push_back(0);
    for (uint64_t i = 0; i < n; ++i) {
        t.off.push_back(t.off.back() + (rnd() % 3 == 0 ? 0 : rnd() % (maxlen + 1)));
        t.slot.push_back((uint32_t)(rnd() % 4));
    }
    return t;
}

// B from A: the same spans with some merged, split or given another slot, and
// the end cut off or grown, so that boundaries coincide often.
Table vary(const Table &a, uint64_t maxlen) {
    Table t;
    t.off.push_back(0);
    for (uint64_t i = 0; i < a.n(); ++i) {
        const uint64_t len = a.off[i + 1] - a.off[i];
        const uint64_t kind = rnd() % 8;
        if (kind == 0 && len > 1) {  // split
            const uint64_t cut = 1 + rnd() % (len - 1);
            t.off.push_back(t.off.back() + cut);
            t.slot.push_back(a.slot[i]);
            t.off.push_back(t.off.back() + len - cut);
            t.slot.push_back((uint32_t)(rnd() % 4));
        } else if (kind == 1 && !t.slot.empty()) {  // merge into the span before
            t.off.back() += len;
        } else {
            t.off.push_back(t.off.back() + len);
            t.slot.push_back(kind == 2 ? (uint32_t)(rnd() % 4) : a.slot[i]);
        }
        if (rnd() % 6 == 0) {  // a span of length 0, at a boundary both have
            t.off.push_back(t.off.back());
            t.slot.push_back((uint32_t)(rnd() % 4));
        }
    }
    if (rnd() % 3 == 0) {
        t.off.push_back(t.off.back() + rnd() % (maxlen + 1));
        t.slot.push_back(9);
    } else if (rnd() % 3 == 0 && t.n() > 1) {
        t.off.pop_back();
        t.slot.pop_back();
    }
    return t;
}

struct Piece {
    uint64_t x, end;
    uint32_t ia, ib;
    bool shared;
};

// Stages 1 and 2 with the header's functions, checked against brute force.
std::vector<Piece> pieces_of(const Table &a, const Table &b) {
    const uint64_t common = a.size() < b.size() ? a.size() : b.size();
    std::vector<Piece> out;
    if (!common) return out;
    const uint64_t nc = cdc::diff_candidates(a.n(), b.n());
    uint64_t *scan = static_cast<uint64_t *>(std::malloc((nc + 1) * sizeof(uint64_t)));
    scan[0] = 0;
    for (uint64_t c = 0; c < nc; ++c) {
        uint64_t x = 0;
        scan[c + 1] = scan[c] + (cdc::diff_opens(a.off.data(), a.n(), b.off.data(), b.n(), common, c, &x) ? 1 : 0);
    }
    const uint64_t P = scan[nc];
    out.resize(P);
    std::vector<int> hit(P, 0);
    for (uint64_t c = 0; c < nc; ++c) {
        uint64_t x = 0;
        if (!cdc::diff_opens(a.off.data(), a.n(), b.off.data(), b.n(), common, c, &x)) continue;
        uint32_t ia = 0, ib = 0;
        const uint64_t p = cdc::diff_rank(a.off.data(), a.n(), b.off.data(), b.n(), scan, c, x, &ia, &ib);
        CHECK(p < P);
        if (p >= P) continue;
        ++hit[p];
        out[p] = Piece{x, 0, ia, ib, false};
    }
    std::free(scan);
    // Brute force: the distinct boundaries below common, ascending.
    std::vector<uint64_t> want;
    for (uint64_t x = 0; x < common; ++x) {
        bool is = false;
        for (uint64_t v : a.off) is = is || v == x;
        for (uint64_t v : b.off) is = is || v == x;
        if (is) want.push_back(x);
    }
    CHECK(want.size() == P);
    for (uint64_t p = 0; p < P && p < want.size(); ++p) {
        Piece &pc = out[p];
        CHECK(hit[p] == 1);
        CHECK(pc.x == want[p]);
        pc.end = p + 1 < P ? want[p + 1] : common;
        CHECK(pc.ia < a.n() && a.off[pc.ia] <= pc.x && pc.end <= a.off[pc.ia + 1]);
        CHECK(pc.ib < b.n() && b.off[pc.ib] <= pc.x && pc.end <= b.off[pc.ib + 1]);
        if (pc.ia >= a.n() || pc.ib >= b.n()) continue;
        pc.shared = cdc::diff_shared(a.slot[pc.ia], a.off[pc.ia], b.slot[pc.ib], b.off[pc.ib]);
    }
    return out;
}

Ranges brute(const std::vector<uint8_t> &diff) {
    Ranges r;
    for (uint64_t x = 0; x < diff.size(); ++x)
        if (diff[x]) {
            if (!r.empty() && r.back().first + r.back().second == x) ++r.back().second;
            else r.push_back({x, 1});
        }
    return r;
}

// Stages 3 and 4 on the host: diff[x] for x < common says whether the bytes
// differ (never inside a shared piece); past common everything differs.
Ranges runs_of(const std::vector<Piece> &pieces, const std::vector<uint8_t> &diff, uint64_t common, uint64_t maxsz) {
    struct Cmp {
        uint64_t x, len, t0;
        uint32_t m, flag;
    };
    const bool tail = maxsz != common;
    std::vector<Cmp> cp;
    uint64_t tiles = 0;
    for (uint64_t p = 0; p < pieces.size(); ++p) {
        if (pieces[p].shared) continue;
        const uint32_t m = (uint32_t)(rnd() % 16);
        const uint64_t len = pieces[p].end - pieces[p].x;
        const uint32_t flag = (p > 0 && !pieces[p - 1].shared ? 1u : 0u) | (pieces[p].end == common && tail ? 2u : 0u);
        cp.push_back(Cmp{pieces[p].x, len, tiles, m, flag});
        tiles += cdc::diff_tiles(m, len);
    }
    const uint64_t W = cdc::kDiffTileWords;
    uint64_t *mask = static_cast<uint64_t *>(std::calloc(tiles * W + 1, sizeof(uint64_t)));
    for (const Cmp &c : cp)
        for (uint64_t i = 0; i < c.len; ++i)
            if (diff[c.x + i]) {
                const uint64_t bit = c.t0 * cdc::kDiffTile + c.m + i;
                mask[bit / 64] |= 1ull << (bit % 64);
            }
    auto bit_at = [&](uint64_t tile, uint32_t b) { return (mask[tile * W + b / 64] >> (b % 64)) & 1; };
    auto last_bit = [&](const Cmp &c) {
        uint64_t k;
        uint32_t b;
        cdc::diff_last_bit(c.m, c.len, &k, &b);
        return bit_at(c.t0 + k, b);
    };
    auto tile_at = [&](uint64_t ci, uint64_t k) {
        const Cmp &c = cp[ci];
        cdc::DiffTile t;
        t.m = c.m;
        t.len = c.len;
        t.k = k;
        t.head_joined = k == 0 && (c.flag & 1u) && last_bit(cp[ci - 1]);
        t.tail_joined = false;
        if (k + 1 == cdc::diff_tiles(c.m, c.len))
            t.tail_joined = (c.flag & 2u) ||
                            (ci + 1 < cp.size() && (cp[ci + 1].flag & 1u) && bit_at(cp[ci + 1].t0, cp[ci + 1].m));
        return t;
    };
    // Starts per tile and their scan.
    std::vector<uint64_t> tcount(tiles + 1, 0);
    for (uint64_t ci = 0; ci < cp.size(); ++ci)
        for (uint64_t k = 0; k < cdc::diff_tiles(cp[ci].m, cp[ci].len); ++k) {
            const uint64_t T = cp[ci].t0 + k;
            const cdc::DiffTile t = tile_at(ci, k);
            uint64_t n = 0;
            for (uint32_t l = 0; l < W; ++l) {
                const uint64_t prev = l ? mask[T * W + l - 1] >> 63 : (k ? mask[T * W - 1] >> 63 : 0);
                n += (uint64_t)__builtin_popcountll(cdc::diff_tile_starts(t, l, mask[T * W + l], prev));
            }
            tcount[T + 1] = n;
        }
    for (uint64_t T = 0; T < tiles; ++T) tcount[T + 1] += tcount[T];
    const uint64_t S = tcount[tiles];
    const bool joined = tail && !cp.empty() && (cp.back().flag & 2u) && last_bit(cp.back());
    const uint64_t R = S + (tail && !joined ? 1 : 0);
    std::pair<uint64_t, uint64_t> *out =
        static_cast<std::pair<uint64_t, uint64_t> *>(std::calloc(R + 1, sizeof(std::pair<uint64_t, uint64_t>)));
    std::vector<int> wrote_s(R, 0), wrote_e(R, 0);
    if (tail) {
        if (joined) out[R - 1].second = maxsz;
        else out[R - 1] = {common, maxsz}, ++wrote_s[R - 1];
        ++wrote_e[R - 1];
    }
    for (uint64_t ci = 0; ci < cp.size(); ++ci)
        for (uint64_t k = 0; k < cdc::diff_tiles(cp[ci].m, cp[ci].len); ++k) {
            const uint64_t T = cp[ci].t0 + k;
            const cdc::DiffTile t = tile_at(ci, k);
            uint64_t rs = tcount[T], re = 0;
            for (uint32_t l = 0; l < W; ++l) {
                const uint64_t w = mask[T * W + l];
                const uint64_t prev = l ? mask[T * W + l - 1] >> 63 : (k ? mask[T * W - 1] >> 63 : 0);
                const uint64_t next = l + 1 < W ? mask[T * W + l + 1] & 1
                                                : (k + 1 < cdc::diff_tiles(t.m, t.len) ? mask[(T + 1) * W] & 1 : 0);
                uint64_t starts = cdc::diff_tile_starts(t, l, w, prev), ends = cdc::diff_tile_ends(t, l, w, next);
                if (l == 0) re = tcount[T] - cdc::diff_tile_open(t, w, starts);
                for (; starts; starts &= starts - 1) {
                    CHECK(rs < R);
                    if (rs >= R) break;
                    ++wrote_s[rs];
                    out[rs++].first =
                        cdc::diff_file_offset(cp[ci].x, t.m, k, l * 64 + (uint32_t)__builtin_ctzll(starts));
                }
                for (; ends; ends &= ends - 1) {
                    CHECK(re < R);
                    if (re >= R) break;
                    ++wrote_e[re];
                    out[re++].second =
                        cdc::diff_file_offset(cp[ci].x, t.m, k, l * 64 + (uint32_t)__builtin_ctzll(ends)) + 1;
                }
            }
        }
    Ranges r;
    for (uint64_t i = 0; i < R; ++i) {
        CHECK(wrote_s[i] == 1 && wrote_e[i] == 1);
        r.push_back({out[i].first, out[i].second - out[i].first});
    }
    std::free(out);
    std::free(mask);
    return r;
}

void check_pair(const Table &a, const Table &b, int density) {
    const std::vector<Piece> pieces = pieces_of(a, b);
    const uint64_t common = a.size() < b.size() ? a.size() : b.size();
    const uint64_t maxsz = a.size() < b.size() ? b.size() : a.size();
    std::vector<uint8_t> diff(maxsz, 1);
    for (const Piece &pc : pieces)
        for (uint64_t x = pc.x; x < pc.end; ++x)
            diff[x] = pc.shared ? 0 : density == 0 ? 0 : density == 1 ? 1 : density == 2 ? (x & 1) : rnd() % density == 0;
    // The bytes next to every piece border, both ways: the carries' cases.
    if (density > 2)
        for (const Piece &pc : pieces)
            if (!pc.shared) {
                if (rnd() % 2) diff[pc.x] = 1;
                if (rnd() % 2) diff[pc.end - 1] = 1;
            }
    const Ranges got = runs_of(pieces, diff, common, maxsz), want = brute(diff);
    CHECK(got == want);
}

void check_words() {
    for (int t = 0; t < 20000; ++t) {
        const uint64_t w = t < 4 ? (t & 1 ? ~0ull : 0) : rnd() & rnd(), prev = rnd() & 1, next = rnd() & 1;
        uint64_t s = 0, e = 0;
        for (int b = 0; b < 64; ++b) {
            const uint64_t cur = (w >> b) & 1, before = b ? (w >> (b - 1)) & 1 : prev,
                           after = b < 63 ? (w >> (b + 1)) & 1 : next;
            if (cur && !before) s |= 1ull << b;
            if (cur && !after) e |= 1ull << b;
        }
        CHECK(cdc::diff_word_starts(w, prev) == s);
        CHECK(cdc::diff_word_ends(w, next) == e);
    }
    // Tiles and the bit <-> byte map.
    for (uint32_t m = 0; m < 16; ++m)
        for (uint64_t len : {1ull, 15ull, 16ull, 17ull, 4080ull, 4081ull, 4095ull, 4096ull, 4097ull, 8193ull, 12288ull}) {
            const uint64_t tiles = cdc::diff_tiles(0x1000 + m, len);
            CHECK(tiles == (m + len + 4095) / 4096);
            uint64_t k;
            uint32_t b;
            cdc::diff_last_bit(m, len, &k, &b);
            CHECK(k == tiles - 1 && cdc::diff_file_offset(77, m, k, b) == 77 + len - 1);
            CHECK(cdc::diff_file_offset(77, m, 0, m) == 77);
        }
    CHECK(cdc::diff_tiles(5, 0) == 0);
}

}  // namespace

int main() {
    check_words();
    for (int t = 0; t < 1500; ++t) {
        const uint64_t na = t < 10 ? (uint64_t)t : rnd() % 40;
        const uint64_t maxlen = t % 50 == 49 ? 9000 : t % 7 == 0 ? 200 : 20;
        const Table a = make_table(na, maxlen);
        const Table b = t % 3 == 0 ? make_table(rnd() % 40, maxlen) : vary(a, maxlen);
        for (int density : {0, 1, 2, 3, 9}) check_pair(a, b, density);
        if (t % 5 == 0) check_pair(a, a, 1), check_pair(b, a, 3);
    }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::puts("diff plan ok");
    return 0;
}
