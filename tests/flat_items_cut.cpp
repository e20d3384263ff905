// Host check of csrc/flat_items.h (built by test_flat_items_host.py with ASan and UBSan): the chunk rules against literals
// worked out by hand from the formulas the kernels have always used, and the cutter on seeded lists of totals.
#include "flat_items.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace cyb_flat;

static int failures = 0;

#define EXPECT(cond, ...)                                                                                                                  \
    do {                                                                                                                                   \
        if (!(cond)) {                                                                                                                     \
            if (++failures <= 20) std::printf("MISMATCH %s:%d: ", __FILE__, __LINE__), std::printf(__VA_ARGS__), std::printf("\n");        \
        }                                                                                                                                  \
    } while (0)

struct Lit {
    int64_t total, chunk;
};

static void check_literals(const char* name, int64_t (*rule)(int64_t), const std::vector<Lit>& lits)
{
    for (const Lit& l : lits)
        EXPECT(rule(l.total) == l.chunk, "%s(%lld) = %lld, expected %lld", name, (long long)l.total, (long long)rule(l.total), (long long)l.chunk);
}

// the items of `totals` cut at `chunk`: every record covered exactly once, ascending, no item longer than the chunk
static void check_cover(const char* name, const std::vector<int64_t>& totals, int64_t chunk)
{
    std::vector<Item> items;
    EXPECT(cut(items, totals, chunk), "%s: cut refused a small list", name);
    size_t k = 0;
    for (size_t i = 0; i < totals.size(); ++i) {
        int64_t next = 0;
        while (k < items.size() && items[k].desc == (int32_t)i) {
            const Item& it = items[k++];
            EXPECT(it.pad == 0, "%s: item %zu: pad %d", name, k - 1, it.pad);
            EXPECT(it.start == next, "%s: record %zu: item starts at %lld, expected %lld", name, i, (long long)it.start, (long long)next);
            EXPECT(it.count >= 1 && it.count <= chunk, "%s: record %zu: item of %lld elements, chunk %lld", name, i, (long long)it.count, (long long)chunk);
            // every item but the last of its record is a full chunk
            EXPECT(it.count == chunk || it.start + it.count == totals[i], "%s: record %zu: short item inside the record", name, i);
            next = it.start + it.count;
        }
        EXPECT(next == totals[i], "%s: record %zu: covered up to %lld of %lld", name, i, (long long)next, (long long)totals[i]);
    }
    EXPECT(k == items.size(), "%s: %zu items beyond the last record (or out of order)", name, items.size() - k);
}

// seeded lists whose chunk under `rule` is c, with the edge totals of c among them; `bulk` elements in one further record steer
// the sum (and with it the chunk)
static void check_rule(const char* name, int64_t (*rule)(int64_t), int64_t bulk, unsigned seed)
{
    std::mt19937_64 rng(seed);
    int64_t c = rule(bulk);
    for (int round = 0; round < 8; ++round) {
        std::vector<int64_t> totals = {0, 1, c - 1, c, c + 1, 2 * c + 1};
        for (int i = 0; i < 24; ++i) totals.push_back((int64_t)(rng() % (uint64_t)(3 * c)));
        if (bulk) totals.push_back(bulk);
        std::shuffle(totals.begin(), totals.end(), rng);
        const int64_t now = rule(sum_of(totals));
        if (now != c) { // the edge totals moved the sum across a step of the rule: take the new chunk's edges
            c = now;
            continue;
        }
        check_cover(name, totals, c);
        return;
    }
    EXPECT(false, "%s: no list with a stable chunk near %lld", name, (long long)bulk);
}

static int64_t fixed_max(int64_t) { return kMaxChunk; }
static int64_t tiles4(int64_t) { return 4; }
static int64_t tiles16(int64_t) { return 16; }

int main()
{
    const int64_t K = 2048;
    // real rule: total / 2048 rounded up to a multiple of 1024, inside 8192 .. 65536
    check_literals("chunk_real", chunk_real,
                   {{0, 8192}, {1, 8192}, {K * 8192, 8192}, {K * 8192 + 2047, 8192}, {K * 8193, 9216}, {K * 9216 + 2047, 9216}, {K * 9217, 10240},
                    {K * 64512, 64512}, {K * 64513, 65536}, {K * 65536, 65536}, {K * 65537, 65536}, {(int64_t)1 << 40, 65536}});
    // complex rule: total / 2048 rounded up to a multiple of 512, inside 4096 .. 32768
    check_literals("chunk_complex", chunk_complex,
                   {{0, 4096}, {1, 4096}, {K * 4096, 4096}, {K * 4096 + 2047, 4096}, {K * 4097, 4608}, {K * 4608 + 2047, 4608}, {K * 4609, 5120},
                    {K * 32256, 32256}, {K * 32257, 32768}, {K * 32768, 32768}, {K * 32769, 32768}, {(int64_t)1 << 40, 32768}});
    // the two rules are not each other's halves: 2048 * 4608 + 1024 complex numbers are 2048 * 9217 doubles
    check_literals("chunk_complex", chunk_complex, {{K * 4608 + 1024, 4608}});
    check_literals("chunk_real", chunk_real, {{2 * (K * 4608 + 1024), 10240}});

    unsigned seed = 1;
    for (int64_t bulk : {(int64_t)0, K * 9000, K * 30000, K * 70000}) {
        check_rule("chunk_real", chunk_real, bulk, seed++);
        check_rule("chunk_complex", chunk_complex, bulk / 2, seed++);
    }
    check_rule("kMaxChunk", fixed_max, 0, seed++);
    check_rule("4 tiles", tiles4, 0, seed++);
    check_rule("16 tiles", tiles16, 0, seed++);

    // empty lists, and items appended behind those of an earlier cut
    check_cover("empty", {}, 8192);
    check_cover("zeros", {0, 0, 0}, 8192);
    {
        std::vector<Item> items;
        EXPECT(cut(items, {5, 0, 3}, 4) && items.size() == 3, "append: first cut");
        EXPECT(cut(items, {9}, 4) && items.size() == 6 && items[3].desc == 0 && items[5].start == 8 && items[5].count == 1, "append: second cut");
    }
    // a grid is 32 bits wide: 2^31 items are refused before anything is allocated
    {
        std::vector<Item> items;
        EXPECT(!cut(items, {((int64_t)1 << 31) * 4}, 4) && items.empty(), "2^31 items were not refused");
        EXPECT(!cut(items, {((int64_t)1 << 30) * 16, 0, ((int64_t)1 << 30) * 16}, 16) && items.empty(), "2^31 items over two records were not refused");
    }
    if (failures) {
        std::printf("%d mismatches\n", failures);
        return 1;
    }
    std::printf("no mismatch\n");
    return 0;
}
