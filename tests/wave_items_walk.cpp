// Walks the work items of csrc/wave_items.h on the host: every lane of every item, with the shared start and advance, against
// plain division of the flat index.  Built and run by test_wave_items_host.py under ASan and UBSan; exit status 0 = no
// mismatch, and every unit of every record visited exactly once.
#include "wave_items.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace cyb_items;

namespace {

long long g_units = 0, g_records = 0;

#define WALK_REQUIRE(cond, ...)                  \
    do {                                         \
        if (!(cond)) {                           \
            std::fprintf(stderr, "FAIL: ");      \
            std::fprintf(stderr, __VA_ARGS__);   \
            std::fprintf(stderr, "\n");          \
            std::exit(1);                        \
        }                                        \
    } while (0)

template <int L, int S> struct Rec {
    Levels<L, S> lv;
};

// a record whose used levels first .. L - 1 have the given extents; seeded strides: small ones of either sign, zeros, and
// ones beyond 32 bits
template <int L, int S> Rec<L, S> make_rec(std::mt19937_64& rng, int first, const std::vector<int64_t>& ext)
{
    Rec<L, S> r;
    std::memset(&r, 0x5a, sizeof(r)); // set_steps has to fill whatever a kernel reads below `first`
    for (int l = first; l < L; ++l) {
        r.lv.ext[l] = (int32_t)ext[(size_t)(l - first)];
        for (int a = 0; a < S; ++a) {
            const int kind = (int)(rng() % 8);
            const int64_t small = (int64_t)(rng() % 15) - 7;
            r.lv.st[a][l] = kind == 0 ? 0 : (kind == 1 ? small * ((int64_t)1 << 33) : small);
        }
    }
    set_steps(r.lv, first);
    return r;
}

// cuts the list, walks it with the cursor over the levels dev_first .. L - 1 (the record's own first level, or 0: a kernel
// that walks the unused levels too) and compares every unit with division
template <int L, int S> void walk(const std::vector<Rec<L, S>>& recs, bool all_levels, const char* what)
{
    std::vector<int64_t> totals;
    for (const auto& r : recs) {
        int64_t t = 1;
        for (int l = 0; l < L; ++l) {
            WALK_REQUIRE(l >= r.lv.first || r.lv.ext[l] == 1, "%s: level %d below first has extent %d", what, l, (int)r.lv.ext[l]);
            t *= r.lv.ext[l];
        }
        totals.push_back(t);
    }
    const int64_t chunk = chunk_for(totals);
    WALK_REQUIRE(chunk >= kMinChunk && chunk <= kMaxChunk && chunk % WAVE == 0, "%s: chunk %lld", what, (long long)chunk);
    std::vector<Item<L, S>> items;
    cut_items(items, recs, totals);
    size_t at = 0;
    for (size_t i = 0; i < recs.size(); ++i) {
        const Levels<L, S>& t = recs[i].lv;
        const int dev_first = all_levels ? 0 : t.first;
        std::vector<unsigned char> seen((size_t)totals[i], 0);
        for (int64_t e0 = 0; e0 < totals[i]; e0 += chunk, ++at) {
            WALK_REQUIRE(at < items.size(), "%s: record %zu: items missing", what, i);
            const Item<L, S>& it = items[at];
            WALK_REQUIRE(it.rec == (int32_t)i && it.count == std::min(chunk, totals[i] - e0), "%s: record %zu: item %zu has rec %d, count %lld", what, i,
                         at, (int)it.rec, (long long)it.count);
            for (int lane = 0; lane < WAVE; ++lane) {
                Cursor<L, S> c;
                start(c, t, it.at, lane, dev_first);
                for (int64_t k = lane; k < it.count; k += WAVE) {
                    int64_t e = e0 + k;
                    WALK_REQUIRE(++seen[(size_t)e] == 1, "%s: record %zu: unit %lld visited twice", what, i, (long long)(e0 + k));
                    int64_t off[S] = {};
                    for (int l = L - 1; l >= 0; --l) {
                        const int64_t digit = l >= t.first ? e % t.ext[l] : 0;
                        if (l >= t.first) e /= t.ext[l];
                        WALK_REQUIRE(c.idx[l] == digit, "%s: record %zu: unit %lld lane %d: digit %d is %d, not %lld", what, i, (long long)(e0 + k), lane,
                                     l, (int)c.idx[l], (long long)digit);
                        for (int a = 0; a < S; ++a) off[a] += l >= t.first ? digit * t.st[a][l] : 0;
                    }
                    for (int a = 0; a < S; ++a)
                        WALK_REQUIRE(c.off[a] == off[a], "%s: record %zu: unit %lld lane %d: offset %d is %lld, not %lld", what, i, (long long)(e0 + k),
                                     lane, a, (long long)c.off[a], (long long)off[a]);
                    advance(c, t, t.step, t.step_o, dev_first);
                }
            }
        }
        for (int64_t e = 0; e < totals[i]; ++e) WALK_REQUIRE(seen[(size_t)e] == 1, "%s: record %zu: unit %lld not visited", what, i, (long long)e);
        g_units += totals[i];
        ++g_records;
    }
    WALK_REQUIRE(at == items.size(), "%s: %zu items, %zu expected", what, items.size(), at);
}

// `total` as a product of at most `n` factors above 1 (a prime total is one level)
std::vector<int64_t> factors(int64_t total, int n)
{
    std::vector<int64_t> f;
    for (int64_t p = 2; p * p <= total && (int)f.size() + 1 < n; ++p)
        while (total % p == 0 && total > p && (int)f.size() + 1 < n) f.push_back(p), total /= p;
    f.push_back(total);
    return f;
}

template <int L, int S> void run(uint64_t seed, bool all_levels, int64_t big, const char* what)
{
    std::mt19937_64 rng(seed);
    const int64_t kExt[7] = {1, 2, 3, 63, 64, 65, 130};
    const int64_t kTotals[8] = {1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 1};
    // the totals that give a partial wave, a partial last item and more than one item: as one level, and factorised over the
    // last levels with levels of extent 1 between them; a first used level anywhere in the table
    for (int first = 0; first <= L; ++first) {
        std::vector<Rec<L, S>> recs;
        for (int64_t total : kTotals) {
            if (first == L) {
                if (total == 1) recs.push_back(make_rec<L, S>(rng, first, {}));
                continue;
            }
            std::vector<int64_t> one((size_t)(L - first), 1);
            one[(size_t)(rng() % (uint64_t)(L - first))] = total;
            recs.push_back(make_rec<L, S>(rng, first, one));
            std::vector<int64_t> f = factors(total, L - first), many((size_t)(L - first), 1);
            size_t at = many.size();
            for (size_t j = f.size(); j-- > 0;) {
                at -= 1 + (at > j + 1 ? (size_t)(rng() % 2) : 0);
                many[at] = f[j];
            }
            recs.push_back(make_rec<L, S>(rng, first, many));
        }
        // extents where the lane decode clips at WAVE, at most 2 * 10^4 units per record
        for (int n = 0; n < 6 && first < L; ++n) {
            std::vector<int64_t> ext((size_t)(L - first), 1);
            int64_t total = 1;
            for (size_t j = ext.size(); j-- > 0;) {
                const int64_t e = kExt[rng() % 7], small = kExt[rng() % 3];
                ext[j] = total * e <= 20000 ? e : (total * small <= 20000 ? small : 1);
                total *= ext[j];
            }
            recs.push_back(make_rec<L, S>(rng, first, ext));
        }
        walk(recs, all_levels, what);
    }
    // a list whose sum lifts the chunk above kMinChunk: one record of `big` * 65 * 130 units beside small ones
    if (big > 0) {
        std::vector<Rec<L, S>> recs;
        recs.push_back(make_rec<L, S>(rng, L - 1, {2 * 1024 + 1}));
        recs.push_back(make_rec<L, S>(rng, L - 3, {big, 65, 130}));
        recs.push_back(make_rec<L, S>(rng, L - 2, {63, 3}));
        walk(recs, all_levels, what);
    }
}

} // namespace

int main()
{
    // the instantiations of the kernels: tree_outer / tree_compose; tree_place, destination and source; tree_dense, from_dense
    // and to_dense.  1050 * 65 * 130 units lift the chunk to 1088; the cut does not depend on L and S, so one such list does.
    run<4, 1>(1, false, 1050, "<4,1>");
    run<4, 1>(2, true, 0, "<4,1> all levels");
    run<3, 1>(3, false, 0, "<3,1>");
    run<12, 1>(4, false, 0, "<12,1>");
    run<12, 2>(5, true, 0, "<12,2> all levels");
    run<12, 4>(6, true, 0, "<12,4> all levels");
    run<12, 4>(7, false, 0, "<12,4>");
    std::printf("wave_items_walk: %lld records, %lld units: no mismatch\n", g_records, g_units);
    return 0;
}
