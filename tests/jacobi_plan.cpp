// Host check of csrc/jacobi_plan.h (built by test_jacobi_plan_host.py with ASan and UBSan).  The driver of the Jacobi sweep
// kernel sizes its zeroed block, granule regions and descriptor image from this plan and the launch indexes them by it: the walk
// below requires, for every list it builds, that the parts fit, the flag bases and image regions do not overlap, what a plan
// uses never exceeds what was reserved, and the shared-workgroup ranges cover the entries exactly once.  The literals pin
// the parts, the split and the convergence rule to cases worked out by hand from the rule as the driver has always stated it.
//
// Lists: `slots` in {4, 8, 16, 256}; matrices with nb in {2, 4, 6, 8, 28, 40, 92}, lenp in {64, 128, 448, 1472, 4096}, J on / off
// (10 combinations), sorted by falling nb as the driver's work list is.  Lists of 1 - 3 matrices: every list.  Lists of 4 - 6
// matrices are up to 70^6 = 1.2e11, too many to walk: every multiset of nb, and on each the 40 assignments
// (lenp, J)[i] = combination (a + b i) mod 10, b in {0, 1, 3, 7} -- b = 0 gives every list whose matrices share lenp and J.
// The exchange without granules changes two sizes of the layout only: it is walked on the lists of one and two matrices.
#include "jacobi_plan.h"

#include <cstdio>

using namespace cyb;

static int failures = 0;
static long lists = 0;

#define EXPECT(cond, ...)                                                                                                                  \
    do {                                                                                                                                   \
        if (!(cond)) {                                                                                                                     \
            if (++failures <= 20) std::printf("MISMATCH %s:%d: ", __FILE__, __LINE__), std::printf(__VA_ARGS__), std::printf("\n");        \
        }                                                                                                                                  \
    } while (0)

static const int kNb[] = {2, 4, 6, 8, 28, 40, 92};
static const int kLenp[] = {64, 128, 448, 1472, 4096};
static const size_t kHead = 48; // convergence words + error word of a small call (a multiple of 16)

static PlanMat make_mat(int nb, int combo) { return PlanMat{nb, 16 * nb, kLenp[combo % 5], combo >= 5}; }

static void check_list(const std::vector<PlanMat>& mats, size_t slots)
{
    ++lists;
    for (int gran = mats.size() <= 2 ? 0 : 1; gran < 2; ++gran) {
        const SweepPlan p = plan_sweep(mats, slots, 0, kHead, gran != 0);
        const SweepLayout& L = p.layout;
        // (a) parts
        size_t total = 0, np = 0, ready = 0, reserved = 0;
        bool all_one = true;
        for (size_t i = 0; i < mats.size(); ++i) {
            const int g = p.G[i];
            EXPECT(g >= 1 && g <= std::min(RGMAX, std::max(1, mats[i].lenp / 64)), "matrix %zu (nb %d lenp %d): %d parts", i, mats[i].nb, mats[i].lenp, g);
            total += (size_t)mats[i].nb / 2 * (size_t)g;
            np += (size_t)mats[i].nb / 2;
            ready += (size_t)mats[i].nb * (size_t)g;
            reserved += (size_t)mats[i].nb * RGMAX;
            all_one = all_one && g == 1;
        }
        EXPECT(total <= slots || all_one, "%zu entries on %zu slots with more than one part somewhere", total, slots);
        EXPECT(L.fits, "a plan without CYB_JACOBI_G always fits");
        EXPECT(L.np == np && L.entries == total, "layout counts %zu pairs %zu entries, expected %zu %zu", L.np, L.entries, np, total);
        // (b) layout: flag bases
        EXPECT(L.flag_base.size() == mats.size(), "flag bases");
        size_t next = np;
        for (size_t i = 0; i < mats.size() && i < L.flag_base.size(); ++i) {
            EXPECT((size_t)L.flag_base[i] == next, "matrix %zu: flag base %d, expected %zu", i, L.flag_base[i], next);
            next += (size_t)mats[i].nb * (size_t)p.G[i];
        }
        EXPECT(L.ready_used == ready && L.ready_reserved == reserved && ready <= reserved, "ready counters: %zu used, %zu reserved", L.ready_used, L.ready_reserved);
        // every counter the kernel indexes (tickets [0, np), ready W and ready J at the flag bases) lies inside the zeroed block
        EXPECT(4 * (L.ready_reserved + np + L.ready_used) <= L.ready_bytes, "ready J runs past the zeroed block");
        EXPECT(L.zero_bytes == kHead + L.ready_bytes && L.ready_bytes % 16 == 0, "zeroed block");
        // granule regions
        EXPECT(L.gran_used <= L.gran_reserved, "granules: %zu bytes used, %zu reserved (slots %zu)", L.gran_used, L.gran_reserved, slots);
        EXPECT(L.gran_reserved == (gran ? 2 * kPlanGranBytes * slots : 0), "granules reserved");
        EXPECT(L.gran_used == ((gran && !all_one) ? ready * kPlanGranBytes : 0), "granules in use: %zu", L.gran_used);
        if (all_one) EXPECT(L.gran_used == 0, "no matrix has more than one part, yet %zu granule bytes", L.gran_used);
        // descriptor image
        EXPECT(L.map_off % 256 == 0 && L.ent_off % 256 == 0, "image offsets %zu %zu", L.map_off, L.ent_off);
        EXPECT(L.map_off >= kPlanPairBytes * np && L.ent_off >= L.map_off + kPlanMapBytes * total &&
                   L.image_bytes == L.ent_off + kPlanMapBytes * p.share.ranges.size(),
               "image regions overlap: %zu %zu %zu", L.map_off, L.ent_off, L.image_bytes);
        // (c) sharing
        const std::vector<PlanRange>& rg = p.share.ranges;
        if (total <= slots) EXPECT(rg.empty(), "%zu entries fit %zu slots, yet %zu ranges", total, slots, rg.size());
        else {
            EXPECT(!rg.empty() && rg.size() <= slots, "%zu workgroups on %zu slots", rg.size(), slots);
            int at = 0;
            for (const PlanRange& r : rg) {
                EXPECT(r.begin == at && r.end > r.begin, "range [%d, %d) behind %d", r.begin, r.end, at);
                at = r.end;
            }
            EXPECT((size_t)at == total, "ranges end at %d of %zu entries", at, total);
            size_t own = 0; // entries of the matrices in front of the split point: one workgroup each
            for (size_t i = 0; i < p.share.split && i < mats.size(); ++i) own += (size_t)mats[i].nb / 2;
            for (size_t e = 0; e < own && e < rg.size(); ++e) EXPECT(rg[e].begin == (int)e && rg[e].end == (int)e + 1, "entry %zu in front of the split shares", e);
            for (size_t w = own; w < rg.size(); ++w) EXPECT((size_t)(rg[w].end - rg[w].begin) <= p.share.per_wg, "workgroup %zu runs more than %zu entries", w, p.share.per_wg);
        }
    }
}

static void walk(std::vector<PlanMat>& mats, std::vector<int>& nbs, size_t len, int nb_from)
{   // every multiset of nb, falling as in the work list, then the (lenp, J) assignments
    if (nbs.size() == len) {
        auto run = [&]() {
            for (size_t slots : {4, 8, 16, 256}) check_list(mats, slots);
        };
        if (len <= 3) { // every assignment (equal nb keep the order of the list, as under the driver's stable sort)
            size_t n_assign = 1;
            for (size_t i = 0; i < len; ++i) n_assign *= 10;
            for (size_t c = 0; c < n_assign; ++c) {
                mats.clear();
                size_t d = c;
                for (size_t i = 0; i < len; ++i, d /= 10) mats.push_back(make_mat(nbs[i], (int)(d % 10)));
                run();
            }
        } else
            for (int a = 0; a < 10; ++a)
                for (int b : {0, 1, 3, 7}) {
                    mats.clear();
                    for (size_t i = 0; i < len; ++i) mats.push_back(make_mat(nbs[i], (a + b * (int)i) % 10));
                    run();
                }
        return;
    }
    for (int k = nb_from; k >= 0; --k) {
        nbs.push_back(kNb[k]);
        walk(mats, nbs, len, k);
        nbs.pop_back();
    }
}

int main()
{
    std::vector<PlanMat> mats;
    std::vector<int> nbs;
    for (size_t len = 1; len <= 6; ++len) walk(mats, nbs, len, 6);

    // ---- parts by hand.  One matrix, nb = 4 (2 pairs), 8 column chunks, 8 slots: 2 pairs in use, every further part costs 2 slots:
    // G = 2 (4 used), 3 (6), 4 (8), and a fifth would need 10
    {
        const std::vector<int> G = plan_parts({PlanMat{4, 512, 512, true}}, 8, 0);
        EXPECT(G.size() == 1 && G[0] == 4, "one matrix on 8 slots: G = %d", G[0]);
    }
    // A (nb = 8: 4 pairs, 2 chunks) and B (nb = 4: 2 pairs, 1 chunk) on 16 slots: B has no second chunk to give to a part, A takes
    // one more part (6 + 4 = 10 slots) and then has no third chunk
    {
        const std::vector<int> G = plan_parts({PlanMat{8, 128, 128, true}, PlanMat{4, 64, 64, true}}, 16, 0);
        EXPECT(G.size() == 2 && G[0] == 2 && G[1] == 1, "two matrices on 16 slots: G = (%d, %d)", G[0], G[1]);
    }
    // CYB_JACOBI_G: the override is clamped by RGMAX and by the chunks, whatever the room
    {
        const std::vector<int> G = plan_parts({PlanMat{8, 128, 1472, true}, PlanMat{4, 64, 64, false}}, 4, 16);
        EXPECT(G[0] == 8 && G[1] == 1, "override 16: G = (%d, %d)", G[0], G[1]);
        const SweepLayout L = plan_layout({PlanMat{8, 128, 1472, true}, PlanMat{4, 64, 64, false}}, G, 4, kHead, true, 0);
        EXPECT(!L.fits && L.entries == 34, "34 entries in parts do not fit 4 slots (the driver then takes the split route)");
    }
    // ---- sharing by hand.  Block counts 6 4 4 4: 3 + 2 + 2 + 2 = 9 entries on 4 slots.  Split in front of matrix 0: all 9 entries
    // share 4 workgroups, 3 each: cost max(5, 3 x 5) = 15 rounds.  In front of matrix 1: 3 own workgroups, the other 6 entries on
    // the one left: max(5, 6 x 3) = 18.  In front of matrix 2: 5 own workgroups do not fit.
    {
        const PlanShare sh = plan_share({6, 4, 4, 4}, 9, 4);
        EXPECT(sh.split == 0 && sh.per_wg == 3 && sh.ranges.size() == 3, "split %zu, %zu per workgroup, %zu ranges", sh.split, sh.per_wg, sh.ranges.size());
        for (size_t w = 0; w < sh.ranges.size() && w < 3; ++w)
            EXPECT(sh.ranges[w].begin == 3 * (int)w && sh.ranges[w].end == 3 * (int)w + 3, "range %zu: [%d, %d)", w, sh.ranges[w].begin, sh.ranges[w].end);
        EXPECT(plan_share({6, 4, 4, 4}, 9, 9).ranges.empty() && plan_share({6, 4, 4, 4}, 9, 16).ranges.empty(), "no ranges when the entries fit");
    }
    // one long matrix keeps its workgroups, the short ones share: 28 blocks (14 entries) + eight of 2 blocks (8 entries) on 16
    // slots: in front of matrix 1, 14 own + 8 entries on 2 workgroups, 4 each: max(27, 4 x 1) = 27 against 2 x 27 in front of matrix 0
    {
        const PlanShare sh = plan_share({28, 2, 2, 2, 2, 2, 2, 2, 2}, 22, 16);
        EXPECT(sh.split == 1 && sh.per_wg == 4 && sh.ranges.size() == 16, "long + short: split %zu, %zu per workgroup, %zu ranges", sh.split, sh.per_wg, sh.ranges.size());
    }

    // ---- (d) convergence rule on the recorded histories (tol 3.4e-14; sweeps count from one)
    const double tol = 3.4e-14;
    // chi=4096 list: 1.8e-4 -> 2.3e-9: 2.3e-9 <= sqrt(tol) / 10 = 1.8e-8, <= prev^1.5 = 2.4e-6, <= 16 prev^2 = 5.2e-7: the stop is predicted
    EXPECT(!jacobi_sweep_done(1.8e-4, 3.0e-2, tol, 4), "1.8e-4 is no stop");
    EXPECT(jacobi_predicted(2.3e-9, 1.8e-4, tol) && !jacobi_stagnated(2.3e-9, 1.8e-4, tol, 5) && jacobi_sweep_done(2.3e-9, 1.8e-4, tol, 5), "1.8e-4 -> 2.3e-9: predicted stop");
    EXPECT(!jacobi_sweep_done(2.3e-9, 1.8e-4, tol, 5, false), "... but not without prediction");
    // seed 301: 5.0e-7 -> 3.2e-10 is superlinear (<= prev^1.5 = 3.5e-10) but 1280 prev^2: no predicted stop; 3.2e-10 -> 1.6e-10 neither
    EXPECT(!jacobi_predicted(3.2e-10, 5.0e-7, tol) && !jacobi_sweep_done(3.2e-10, 5.0e-7, tol, 5), "5.0e-7 -> 3.2e-10: no stop");
    EXPECT(!jacobi_predicted(1.6e-10, 3.2e-10, tol) && !jacobi_sweep_done(1.6e-10, 3.2e-10, tol, 6), "3.2e-10 -> 1.6e-10: no stop");
    // linear creep 1.7e-8 -> 4.4e-9: below sqrt(tol) / 10 but not superlinear
    EXPECT(!jacobi_sweep_done(4.4e-9, 1.7e-8, tol, 7), "1.7e-8 -> 4.4e-9: no stop");
    // stagnation: within 64 tol and no longer halving, from sweep 6 on
    EXPECT(jacobi_stagnated(1.0e-12, 1.5e-12, tol, 6) && jacobi_sweep_done(1.0e-12, 1.5e-12, tol, 6, false), "stagnated at sweep 6");
    EXPECT(!jacobi_stagnated(1.0e-12, 1.5e-12, tol, 5) && !jacobi_sweep_done(1.0e-12, 1.5e-12, tol, 5), "not before sweep 6");
    EXPECT(!jacobi_stagnated(1.0e-12, 2.1e-12, tol, 8) && !jacobi_stagnated(3.0e-12, 3.1e-12, tol, 8), "still halving / further than 64 tol");
    // off <= tol, first sweep included (prev = 1e300: none)
    EXPECT(jacobi_sweep_done(3.4e-14, 1e300, tol, 1) && jacobi_sweep_done(0.0, 1e300, tol, 1) && !jacobi_sweep_done(3.5e-14, 1e300, tol, 1), "off <= tol");

    if (failures) {
        std::printf("%d mismatches\n", failures);
        return 1;
    }
    std::printf("no mismatch (%ld lists)\n", lists);
    return 0;
}
