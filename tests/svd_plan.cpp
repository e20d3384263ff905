// Host check of csrc/svd_plan.h (built by test_svd_plan_host.py with ASan and UBSan).  The driver of the QR-preconditioned SVD
// carves its workspace by svd_layout and copies whole ranges of it on the strength of the layout's contracts; it deflates, routes
// and completes by the plan's rules.  The walk below requires the contracts for every list it builds; the literals pin the
// split, the two route rules, the null-row columns and the list split to cases worked out by hand from the rules as the driver
// has always stated them.
//
// Layout lists: blocks m x n with m, n in {1, 2, 63, 64, 65, 128, 200} (49 shapes: tall, wide, square), auxiliary sizes fixed
// per position in the list and no multiples of 256.  Lists of one and two blocks: every list.  Lists of three to six blocks
// are up to 49^6 = 1.4e10: shape[i] = (a + b i) mod 49 for every a and b in {0, 1, 5, 11, 20} -- b = 0 repeats one shape.
#include "svd_plan.h"

#include <cfloat>
#include <cstdio>
#include <cstring>

using namespace cyb;

static int failures = 0;
static long lists = 0;

#define EXPECT(cond, ...)                                                                                                                  \
    do {                                                                                                                                   \
        if (!(cond)) {                                                                                                                     \
            if (++failures <= 20) std::printf("MISMATCH %s:%d: ", __FILE__, __LINE__), std::printf(__VA_ARGS__), std::printf("\n");        \
        }                                                                                                                                  \
    } while (0)

static const int kExt[] = {1, 2, 63, 64, 65, 128, 200};
static const SvdAux kAux[6] = {{1001, 777, 4097, 37}, {8, 255, 257, 0}, {70000, 1, 513, 1}, {300, 300, 300, 300},
                               {256 * 3 + 1, 5000, 9, 64}, {12345, 6789, 1011, 7}};

static bool header_name(const char* n) { return !strcmp(n, "sig") || !strcmp(n, "bad") || !strcmp(n, "dev") || !strcmp(n, "ctl"); }

static void check_layout(const std::vector<int>& m, const std::vector<int>& n)
{
    ++lists;
    const size_t nmat = m.size();
    const std::vector<SvdAux> aux(kAux, kAux + nmat);
    const SvdLayout lay = svd_layout(m, n, aux);
    EXPECT(lay.nmat() == nmat && lay.total % 256 == 0, "%zu blocks, total %zu", lay.nmat(), lay.total);
    // every region inside the total, pairwise disjoint
    std::vector<SvdRegion> rg = lay.regions;
    std::sort(rg.begin(), rg.end(), [](const SvdRegion& a, const SvdRegion& b) { return a.off < b.off; });
    size_t head_sum = 0;
    for (size_t i = 0; i < rg.size(); ++i) {
        EXPECT(rg[i].bytes > 0 && rg[i].off + rg[i].bytes <= lay.total, "%s of block %d: [%zu, +%zu) outside %zu", rg[i].name, rg[i].block,
               rg[i].off, rg[i].bytes, lay.total);
        if (i + 1 < rg.size())
            EXPECT(rg[i].off + rg[i].bytes <= rg[i + 1].off, "%s of block %d overlaps %s of block %d", rg[i].name, rg[i].block, rg[i + 1].name,
                   rg[i + 1].block);
        const bool in_head = rg[i].off >= lay.head_begin && rg[i].off + rg[i].bytes <= lay.head_begin + lay.head_bytes;
        const bool off_head = rg[i].off >= lay.head_begin + lay.head_bytes || rg[i].off + rg[i].bytes <= lay.head_begin;
        // the header range covers exactly the sig, bad, dev and ctl words
        if (header_name(rg[i].name)) {
            EXPECT(in_head, "%s of block %d outside the header", rg[i].name, rg[i].block);
            head_sum += rg[i].bytes;
        } else {
            EXPECT(off_head, "%s of block %d inside the header", rg[i].name, rg[i].block);
            if (strcmp(rg[i].name, "idx")) EXPECT(rg[i].off % 256 == 0, "%s of block %d at %zu", rg[i].name, rg[i].block, rg[i].off);
        }
    }
    EXPECT(head_sum == lay.head_bytes, "header of %zu bytes holds %zu bytes of words", lay.head_bytes, head_sum);
    EXPECT(rg.size() == 24 * nmat, "%zu regions for %zu blocks", rg.size(), nmat);
    // bad and dev: adjacent arrays of nmat doubles; ctl: two doubles per block
    EXPECT(lay.flags_begin() == lay.blk[0].bad && lay.flags_bytes() == 16 * nmat, "flags range");
    EXPECT(lay.blk[0].dev == lay.blk[0].bad + 8 * nmat, "dev begins at %zu, bad ends at %zu", lay.blk[0].dev, lay.blk[0].bad + 8 * nmat);
    EXPECT(lay.blk[0].ctl == lay.blk[0].dev + 8 * nmat, "ctl begins at %zu", lay.blk[0].ctl);
    EXPECT(lay.idx_begin % 256 == 0, "index lists at %zu", lay.idx_begin);
    size_t idx = lay.idx_begin, sig = lay.head_begin;
    for (size_t b = 0; b < nmat; ++b) {
        const SvdBlockLay& l = lay.blk[b];
        const size_t k = (size_t)std::min(m[b], n[b]), L = (size_t)std::max(m[b], n[b]), kp = (k + 63) / 64 * 64;
        EXPECT(l.m == m[b] && l.n == n[b] && (size_t)l.k == k && (size_t)l.L == L && (size_t)l.kp == kp && l.tall == (m[b] >= n[b]), "extents");
        EXPECT(l.bad == lay.blk[0].bad + 8 * b && l.dev == lay.blk[0].dev + 8 * b && l.ctl == lay.blk[0].ctl + 16 * b, "words of block %zu", b);
        EXPECT(l.sig == sig && lay.head_index(l.sig) + kp <= lay.head_bytes / 8, "sig of block %zu", b);
        sig += 8 * kp;
        // the index lists: contiguous in block order, k entries each
        EXPECT(l.idx == idx, "index list of block %zu at %zu, expected %zu", b, l.idx, idx);
        idx += 4 * k;
        // sizes: what the kernels index
        for (const SvdRegion& r : lay.regions) {
            if (r.block != (int)b) continue;
            size_t want = r.bytes;
            if (!strcmp(r.name, "Ac") || !strcmp(r.name, "Cq")) want = 8 * L * k;
            if (!strcmp(r.name, "W") || !strcmp(r.name, "J") || !strcmp(r.name, "Wc") || !strcmp(r.name, "Jc") || !strcmp(r.name, "Wq")) want = 8 * kp * kp;
            if (!strcmp(r.name, "Fc") || !strcmp(r.name, "Cn") || !strcmp(r.name, "Cq2")) want = 8 * k * k;
            if (!strcmp(r.name, "sig") || !strcmp(r.name, "sig2") || !strcmp(r.name, "sigo")) want = 8 * kp;
            if (!strcmp(r.name, "rank") || !strcmp(r.name, "inv")) want = 4 * kp;
            if (!strcmp(r.name, "nnull")) want = 4;
            if (!strcmp(r.name, "idx")) want = 4 * k;
            if (!strcmp(r.name, "bad") || !strcmp(r.name, "dev")) want = 8;
            if (!strcmp(r.name, "ctl")) want = 16;
            if (!strcmp(r.name, "aux")) want = aux[b].qr1;
            if (!strcmp(r.name, "aux2")) want = aux[b].complete;
            if (!strcmp(r.name, "aux3")) want = aux[b].lq;
            if (!strcmp(r.name, "stop")) want = 8 * std::max<size_t>(1, aux[b].stop_doubles);
            EXPECT(r.bytes == want, "%s of block %zu: %zu bytes, expected %zu", r.name, b, r.bytes, want);
        }
    }
    EXPECT(idx - lay.idx_begin == lay.idx_bytes && idx <= lay.total, "index lists end at %zu", idx);
}

static void walk_layouts()
{
    std::vector<std::pair<int, int>> shape;
    for (int a : kExt)
        for (int b : kExt) shape.push_back({a, b});
    const int ns = (int)shape.size();
    for (int a = 0; a < ns; ++a) {
        check_layout({shape[a].first}, {shape[a].second});
        for (int b = 0; b < ns; ++b) check_layout({shape[a].first, shape[b].first}, {shape[a].second, shape[b].second});
    }
    const int steps[] = {0, 1, 5, 11, 20};
    for (int len = 3; len <= 6; ++len)
        for (int a = 0; a < ns; ++a)
            for (int b : steps) {
                std::vector<int> m, n;
                for (int i = 0; i < len; ++i) {
                    m.push_back(shape[(a + b * i) % ns].first);
                    n.push_back(shape[(a + b * i) % ns].second);
                }
                check_layout(m, n);
            }
}

typedef std::vector<int32_t> Idx;
static bool same(const Idx& a, const Idx& b) { return a == b; }

static void check_split()
{
    // a row norm exactly at the threshold is not kept: the comparison is strict
    const double a[] = {2.0, 1.0, 0.5};
    SvdSplit s = svd_split_rows(a, 3, 1.0, false);
    EXPECT(same(s.good, {0}) && same(s.nul, {1, 2}), "norm at the threshold");
    // the threshold from the norms: ||R||_F^2 (L eps)^2, here 25 * (2 eps)^2 exactly
    const double r[] = {3.0, 4.0};
    EXPECT(svd_rank_thr2(r, 2, 2) == 100.0 * kEps * kEps, "thr2 %.17g", svd_rank_thr2(r, 2, 2));
    EXPECT(kEps == DBL_EPSILON, "eps");
    // an all-zero block: threshold 0, nothing above it, r0 = 0
    const double z[] = {0.0, 0.0, 0.0};
    EXPECT(svd_rank_thr2(z, 3, 7) == 0.0, "threshold of a zero block");
    s = svd_split_rows(z, 3, svd_rank_thr2(z, 3, 7), false);
    EXPECT(s.good.empty() && same(s.nul, {0, 1, 2}), "zero block");
    // an embedded pair with one large and one tiny norm: both kept; a pair of two tiny norms: both dropped
    const double e[] = {1e-20, 1.0, 1e-20, 1e-20};
    s = svd_split_rows(e, 4, 1e-30, true);
    EXPECT(same(s.good, {0, 1}) && same(s.nul, {2, 3}), "embedded pairs");
    s = svd_split_rows(e, 4, 1e-30, false);
    EXPECT(same(s.good, {1}) && same(s.nul, {0, 2, 3}), "the same rows, not embedded");
    // k = 2
    const double t[] = {1.0, 0.0};
    s = svd_split_rows(t, 2, 0.0, false);
    EXPECT(same(s.good, {0}) && same(s.nul, {1}), "k = 2");
    s = svd_split_rows(t, 2, 0.0, true);
    EXPECT(same(s.good, {0, 1}) && s.nul.empty(), "k = 2, one pair");
    const double o[] = {5.0};
    s = svd_split_rows(o, 1, 0.0, false);
    EXPECT(same(s.good, {0}) && s.nul.empty(), "k = 1");
    // after the sweeps (threshold 0) a row is null exactly when its norm is zero: the smallest norm a square root gives
    const double d[] = {sqrt(4.9406564584124654e-324), 0.0};
    s = svd_split_rows(d, 2, 0.0, false);
    EXPECT(same(s.good, {0}) && same(s.nul, {1}), "smallest row norm");
}

static void check_routes()
{
    const SvdSwitches def;
    EXPECT(!def.nolq && !def.lq_always && def.lq_skip_k == 128 && def.lq_skip_ratio == 1e4 && !def.nojrec && def.jrec_ratio == 10.0 &&
               def.jrec_min == 256 && !def.lq_force_redo && !def.jrec_force_redo && !def.trace_redo && !def.noqr && !def.nosmall && !def.nomerge,
           "defaults of the switches");
    EXPECT(JREC_BOUND == 2e-11, "JREC_BOUND");
    EXPECT(jacobi_tol(16) == 16.0 * kEps && jacobi_tol(10000) == 400.0 * kEps && jacobi_tol(1) == 16.0 * kEps, "jacobi_tol");
    const double above4 = nextafter(1e4, 1e5), above1 = nextafter(10.0, 11.0);
    // LQ: a full-rank block of k >= 128 rows with row norms within 1e4 skips it
    EXPECT(wants_lq(127, 127, 1.0, 1.0, def), "k = 127, flat");
    EXPECT(!wants_lq(128, 128, 1.0, 1.0, def), "k = 128, flat");
    EXPECT(!wants_lq(128, 128, 1.0, 1e4, def), "hi = 1e4 lo");
    EXPECT(wants_lq(128, 128, 1.0, above4, def), "hi just above 1e4 lo");
    EXPECT(wants_lq(100, 128, 1.0, 1.0, def), "rank deficient");
    EXPECT(!wants_lq(1, 64, 1.0, 1.0, def) && wants_lq(2, 64, 1.0, 1.0, def), "r0 = 1 / 2");
    EXPECT(!wants_lq(0, 64, 1e300, 0.0, def), "r0 = 0");
    SvdSwitches sw;
    sw.lq_always = true;
    EXPECT(wants_lq(128, 128, 1.0, 1.0, sw) && !wants_lq(1, 64, 1.0, 1.0, sw), "LQ_ALWAYS");
    sw = SvdSwitches();
    sw.nolq = true;
    EXPECT(!wants_lq(100, 128, 1.0, 1.0, sw) && !wants_lq(2, 64, 1.0, 1e9, sw), "NOLQ");
    sw.lq_always = true;
    EXPECT(!wants_lq(100, 128, 1.0, 1.0, sw), "NOLQ and LQ_ALWAYS");
    sw = SvdSwitches();
    sw.lq_skip_k = 2;
    sw.lq_skip_ratio = 1e300;
    EXPECT(!wants_lq(64, 64, 1e-12, 1.0, sw) && wants_lq(63, 64, 1e-12, 1.0, sw), "LQ_SKIP_K = 2, LQ_SKIP_RATIO = 1e300");
    // recovery: an LQ block with at least 256 surviving rows within a factor 10
    EXPECT(!wants_jrec(true, 255, 1.0, 1.0, false, def) && wants_jrec(true, 256, 1.0, 1.0, false, def), "r0 = 255 / 256");
    EXPECT(wants_jrec(true, 512, 1.0, 10.0, false, def) && !wants_jrec(true, 512, 1.0, above1, false, def), "hi = 10 lo and just above");
    EXPECT(!wants_jrec(true, 512, 1.0, 1.0, true, def), "embedded complex");
    EXPECT(!wants_jrec(false, 512, 1.0, 1.0, false, def), "no LQ step");
    sw = SvdSwitches();
    sw.nojrec = true;
    EXPECT(!wants_jrec(true, 512, 1.0, 1.0, false, sw), "NOJREC");
    sw = SvdSwitches();
    sw.jrec_min = 160;
    sw.jrec_ratio = 1e3;
    EXPECT(wants_jrec(true, 160, 1.0, 1e3, false, sw) && !wants_jrec(true, 159, 1.0, 1.0, false, sw), "JREC_MIN, JREC_RATIO");
    // the spread starts empty
    SvdSpread sp;
    EXPECT(sp.lo == 1e300 && sp.hi == 0.0, "empty spread");
    sp.add(3.0);
    sp.add(0.5);
    EXPECT(sp.lo == 0.5 && sp.hi == 3.0, "spread");
}

static void check_null_columns()
{
    // k = 8: rows 2, 5, 7 deflated up front take the trailing columns in order, row 3 (null after the sweeps) its compact position
    const Idx good0 = {0, 1, 3, 4, 6}, nul = {2, 3, 5, 7};
    EXPECT(same(svd_null_columns(good0, nul.data(), 4), {5, 2, 6, 7}), "columns of the null rows");
    // k = 8, every good0 and every set of rows that went null later: distinct columns below k, the compact position for those
    const int k = 8;
    for (int g0 = 0; g0 < (1 << k); ++g0)
        for (int later = g0;; later = (later - 1) & g0) {
            Idx g, nl;
            for (int j = 0; j < k; ++j) {
                if (g0 >> j & 1) g.push_back(j);
                if (!(g0 >> j & 1) || (later >> j & 1)) nl.push_back(j);
            }
            const Idx cols = svd_null_columns(g, nl.data(), (int)nl.size());
            EXPECT(cols.size() == nl.size(), "one column per null row");
            unsigned seen = 0;
            for (size_t q = 0; q < cols.size(); ++q) {
                EXPECT(cols[q] >= 0 && cols[q] < k && !(seen >> cols[q] & 1), "good0 %x later %x: column %d", g0, later, cols[q]);
                seen |= 1u << cols[q];
                if (later >> nl[q] & 1) EXPECT(g[(size_t)cols[q]] == nl[q], "good0 %x: row %d takes column %d", g0, nl[q], cols[q]);
                else EXPECT(cols[q] >= (int)g.size(), "good0 %x: deflated row %d takes column %d", g0, nl[q], cols[q]);
            }
            if (later == 0) break;
        }
    // compact positions
    std::vector<int32_t> pos;
    EXPECT(svd_append_positions(pos, 8, good0) == 0 && same(pos, {0, 1, -1, 2, 3, -1, 4, -1}), "compact positions");
    EXPECT(svd_append_positions(pos, 3, {1}) == 8 && same(pos, {0, 1, -1, 2, 3, -1, 4, -1, -1, 0, -1}), "compact positions, second block");
    EXPECT(svd_append_positions(pos, 2, {}) == 11 && pos.size() == 13 && pos[11] == -1 && pos[12] == -1, "compact positions, r0 = 0");
}

static void check_list_split()
{
    const SvdShape tiny{8, 8, true}, big{140, 140, false}, vec{1, 300, false};
    std::vector<SvdShape> l15(15, tiny), l16(16, tiny);
    l15.push_back(big);
    l16.push_back(big);
    const std::vector<SvdShape> all_tiny(3, tiny), one_vec(1, vec);
    const SvdRoute T = SvdRoute::tiny, D = SvdRoute::direct, P = SvdRoute::pipeline;
    SvdSwitches nomerge, noqr, nosmall;
    nomerge.nomerge = true;
    noqr.noqr = true;
    nosmall.nosmall = true;
    struct Case {
        const char* name;
        const std::vector<SvdShape>* list;
        bool embedded;
        const SvdSwitches* sw;
        SvdRoute small_blocks, last; // route of the fitting blocks (or of the vector), route of the 140 x 140
    };
    const SvdSwitches def;
    const Case cases[] = {
        {"15 tiny + 140", &l15, false, &def, P, P},        {"16 tiny + 140", &l16, false, &def, T, P},
        {"all tiny", &all_tiny, false, &def, T, T},        {"1 x 300", &one_vec, false, &def, D, D},
        {"15 + 140, embedded", &l15, true, &def, P, P},    {"16 + 140, embedded", &l16, true, &def, P, P},
        {"all tiny, embedded", &all_tiny, true, &def, P, P}, {"1 x 300, embedded", &one_vec, true, &def, P, P},
        {"15 + 140, NOMERGE", &l15, false, &nomerge, D, P}, {"16 + 140, NOMERGE", &l16, false, &nomerge, T, P},
        {"all tiny, NOMERGE", &all_tiny, false, &nomerge, T, T}, {"1 x 300, NOMERGE", &one_vec, false, &nomerge, D, D},
        {"15 + 140, NOQR", &l15, false, &noqr, D, D},      {"16 + 140, NOQR", &l16, false, &noqr, T, D},
        {"all tiny, NOQR", &all_tiny, false, &noqr, T, T}, {"1 x 300, NOQR", &one_vec, false, &noqr, D, D},
        {"16 + 140, NOSMALL", &l16, false, &nosmall, P, P}, {"all tiny, NOSMALL", &all_tiny, false, &nosmall, P, P},
    };
    for (const Case& c : cases) {
        const std::vector<SvdRoute> r = svd_split_list(*c.list, c.embedded, *c.sw);
        EXPECT(r.size() == c.list->size(), "%s: %zu routes", c.name, r.size());
        for (size_t i = 0; i < r.size(); ++i) {
            const SvdRoute want = (i + 1 == r.size() && r.size() > 15) ? c.last : c.small_blocks;
            EXPECT(r[i] == want, "%s: block %zu takes route %d, expected %d", c.name, i, (int)r[i], (int)want);
        }
    }
    EXPECT(svd_split_list({}, false, def).empty(), "empty list");
}

int main()
{
    walk_layouts();
    check_split();
    check_routes();
    check_null_columns();
    check_list_split();
    std::printf("%ld layouts walked\n", lists);
    if (failures) {
        std::printf("%d mismatches\n", failures);
        return 1;
    }
    std::printf("no mismatch\n");
    return 0;
}
