// Plan of one persistent Jacobi sweep (jacobi_engine.hip: jacobi_sweep_kernel and its driver): how many column parts every
// matrix's pairs get, which workgroups share entries when the list has more pairs than the chip has workgroups, where the
// counters, the granule regions and the maps of a launch lie, and when a matrix stops sweeping.  The workspace is sized from
// this arithmetic and the launch consumes it, so both take it from ONE SweepLayout; tests/jacobi_plan.cpp walks it on the
// host.  No HIP in here; the switch CYB_JACOBI_G is read in jacobi_engine.hip and arrives as `g_env`.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <math.h>
#include <vector>

#if defined(__HIPCC__)
#define CYB_PLAN_HD __host__ __device__
#else
#define CYB_PLAN_HD
#endif

namespace cyb {

constexpr int RGMAX = 8;                  // most parts per pair
constexpr size_t kPlanGranBytes = 16384;  // one partial Gram as tagged granules (SW_GRAN_BYTES of the sweep kernel)
constexpr size_t kPlanPairBytes = 64;     // one pair descriptor (RPair)
constexpr size_t kPlanMapBytes = 8;       // one entry of the entry map / of the workgroup map (int2)
constexpr double kPredictQuad = 16.0;     // the last sweep is predicted only behind a step with off <= kPredictQuad * prev^2

// ---- convergence rule -----------------------------------------------------------------------------------------------------
// off: the sweep's max |g_ij| / sqrt(g_ii g_jj), prev: that of the sweep before (1e300: none), sweep: ONE-based.
// stagnated: within a small factor of the threshold and no longer falling (rounding floor of the Gram products for long
// vectors).
// predicted: `off` was measured pair by pair BEFORE this sweep rotated the pair.  In the quadratic regime the sweep leaves
// off^2 behind: once off <= sqrt(tol)/10 the rotations just applied have already taken the matrix to the rounding floor and
// another sweep would only re-measure it (chi=4096 list: 1.8e-4 -> 2.3e-9 -> 3.4e-14 in the last three sweeps, tol 3.4e-14)
// ... but only when the decrease is actually superlinear: with clustered singular values the off-norm can creep down
// linearly (1.7e-8 -> 4.4e-9 per sweep was measured) and a sweep is then NOT the last
// ... and only when the last decrease WAS quadratic (off <= kPredictQuad * prev^2): a 128-fold zero eigenvalue (Gram matrix
// of a rank-132 block, scripts/svd_fuzz.py seed 301) went 5.0e-7 -> 3.2e-10 -> 1.6e-10 -> 1.3e-14 -- superlinear by the test
// above, but the rotations inside the cluster (equal norms: large angles on couplings of 1e-10) carry the couplings to the
// other rows from one cluster row to the next instead of annihilating them, and the predicted stop left 1.6e-10 of
// non-orthogonality.  Quadratic steps measured here have off / prev^2 = 0.07 ... 0.2 (chi=4096 list: 1.8e-4 -> 2.3e-9), that
// one 1280.
// predict = false: CYB_JACOBI_NOPREDICT (host loop only: the switch disables the one-launch form, whose test runs on the device).
CYB_PLAN_HD inline bool jacobi_stagnated(double off, double prev, double tol, int sweep)
{
    return sweep >= 6 && off <= 64.0 * tol && off >= 0.5 * prev;
}
CYB_PLAN_HD inline bool jacobi_predicted(double off, double prev, double tol)
{
    return off <= 0.1 * sqrt(tol) && prev < 1.0 && off <= prev * sqrt(prev) && off <= kPredictQuad * prev * prev;
}
// the rule: true when the matrix stops sweeping (converged, stagnated or predicted)
CYB_PLAN_HD inline bool jacobi_sweep_done(double off, double prev, double tol, int sweep, bool predict = true)
{
    const bool stagnated = jacobi_stagnated(off, prev, tol, sweep);
    const bool predicted = predict && jacobi_predicted(off, prev, tol);
    return off <= tol || stagnated || predicted;
}

// ---- parts per pair ---------------------------------------------------------------------------------------------------------
struct PlanMat {   // what the plan needs to know of a matrix, in the order of the work list (more row blocks first)
    int nb, nvp, lenp;
    bool has_j;    // J or rec_j
};

// Parts per pair, matrix by matrix: start with one, then keep giving a workgroup per pair to the matrix whose sweep is the
// longest chain (rounds x per-round work / parts) while the chip has room (`slots` resident workgroups).
// (rec_j: a matrix whose rotations are rebuilt afterwards streams half the columns, but the estimate keeps counting J for it.
//  Its fixed part is too small -- a round of the largest chi=4096 block is 12 us of wait + pivot solve + sort and 6-11 us of
//  exchange whatever G is -- so with the halved width the greedy loop gave that block five parts and every other block one:
//  list 26.5 ms against 24.3 ms with the parts of the accumulating run, 3 / 2 / 1)
// g_env > 0 (CYB_JACOBI_G): that many parts for every matrix that has the columns for them, whatever the room.
inline std::vector<int> plan_parts(const std::vector<PlanMat>& mats, size_t slots, int g_env)
{
    std::vector<int> G(mats.size(), 1);
    auto chain = [&](size_t i) {
        const PlanMat& pm = mats[i];
        const double per_round = 8.0 + 22.0 * (double)(pm.lenp + (pm.has_j ? pm.nvp : 0)) / 2240.0 / (double)G[i]
                                 + (G[i] > 1 ? 4.0 : 0.0); // us: fixed part + MFMA share (+ exchange)
        return per_round * (double)(pm.nb - 1);
    };
    size_t used = 0;
    for (const PlanMat& pm : mats) used += (size_t)pm.nb / 2;
    while (true) {
        int best = -1;
        double worst = 0.0;
        for (size_t i = 0; i < mats.size(); ++i) {
            const PlanMat& pm = mats[i];
            const int cw_ = pm.lenp / 64;
            if (G[i] >= RGMAX || G[i] >= cw_ || used + (size_t)pm.nb / 2 > slots) continue;
            const double c = chain(i);
            if (c > worst) {
                worst = c;
                best = (int)i;
            }
        }
        if (best < 0) break;
        ++G[(size_t)best];
        used += (size_t)mats[(size_t)best].nb / 2;
    }
    if (g_env > 0)
        for (size_t i = 0; i < mats.size(); ++i) G[i] = std::max(1, std::min({g_env, RGMAX, mats[i].lenp / 64}));
    return G;
}

// ---- shared workgroups ------------------------------------------------------------------------------------------------------
struct PlanRange {   // entries [begin, end) of the entry map that one workgroup runs (the device reads it as an int2)
    int begin, end;
};
struct PlanShare {
    size_t split = 0, per_wg = 0;     // matrices in front of position `split` keep a workgroup per entry, the others share per_wg
    std::vector<PlanRange> ranges;    // empty: workgroup b owns entry b
};
// More entries than resident workgroups (a list of many large matrices: 23 hermitian blocks up to 1238^2 have 301 pairs):
// workgroups take several entries and run them one after the other in every round.  A matrix whose pairs sit on shared
// workgroups advances at 1/m of the pace, so the longest chains keep workgroups of their own and the short matrices share:
// split the list (sorted by row blocks) where max(rounds of the longest, m x rounds of the longest shared) is smallest.
// nb: block counts in work-list order; such a list runs every pair in one part, so a matrix has nb / 2 entries.
inline PlanShare plan_share(const std::vector<int>& nb, size_t entries, size_t slots)
{
    PlanShare sh;
    if (entries <= slots) return sh;
    std::vector<size_t> ent_before; // entries of the matrices before position i
    size_t acc = 0;
    for (int b : nb) {
        ent_before.push_back(acc);
        acc += (size_t)b / 2;
    }
    ent_before.push_back(acc);
    double best_cost = 1e300;
    for (size_t i = 0; i <= nb.size(); ++i) {
        const size_t D = ent_before[i], S = acc - D;
        if (D > slots || (S > 0 && D >= slots)) break;
        const size_t m = S ? (S + (slots - D) - 1) / (slots - D) : 1;
        const double own = (double)(nb[0] - 1);
        const double shared = i < nb.size() ? (double)m * (double)(nb[i] - 1) : 0.0;
        const double cost = std::max(own, shared);
        if (cost < best_cost) {
            best_cost = cost;
            sh.split = i;
            sh.per_wg = m;
        }
    }
    const size_t D = ent_before[sh.split];
    for (size_t e = 0; e < D; ++e) sh.ranges.push_back(PlanRange{(int)e, (int)e + 1});
    for (size_t e = D; e < entries; e += sh.per_wg) sh.ranges.push_back(PlanRange{(int)e, (int)std::min(e + sh.per_wg, entries)});
    return sh;
}

// ---- layout -----------------------------------------------------------------------------------------------------------------
// One zeroed block per sweep: [head: off-norm words and error word | one ticket per pair | ready counters of W | ready
// counters of J | granule regions of the parts in use], and one descriptor image: [pair descriptors | entry map | workgroup map].
struct SweepLayout {
    size_t np = 0;                 // pairs of the list: the tickets come first, the ready counters behind them
    std::vector<int> flag_base;    // [matrix, work-list order] first ready counter of the matrix (nb * G of them: [block][part])
    size_t ready_reserved = 0;     // ready counters per array (W, J) the block has room for: nb * RGMAX per matrix
    size_t ready_used = 0;         // ... and those the parts of this plan use: nb * G per matrix
    size_t entries = 0;            // (pair, part) entries: nb / 2 * G per matrix
    size_t ready_bytes = 0;        // [tickets | ready W | ready J]
    size_t zero_bytes = 0;         // head + ready_bytes: the zeroed block without granule regions
    size_t gran_reserved = 0;      // granule regions: room for two (round parity) per resident workgroup ...
    size_t gran_used = 0;          // ... and what this plan's parts use (behind zero_bytes; zeroed with it).  0: no exchange
    size_t map_off = 0, ent_off = 0, image_bytes = 0; // descriptor image
    bool fits = false;             // the entries fit the chip, or every pair runs in one part and workgroups share
};
// head_bytes: what lies in front of the tickets (a multiple of 16); granules: the exchange travels as granules
inline SweepLayout plan_layout(const std::vector<PlanMat>& mats, const std::vector<int>& G, size_t slots, size_t head_bytes, bool granules,
                               size_t n_ranges)
{
    SweepLayout L;
    for (const PlanMat& pm : mats) L.np += (size_t)pm.nb / 2;
    int fb = (int)L.np;
    bool any_parts = false;
    for (size_t i = 0; i < mats.size(); ++i) {
        L.flag_base.push_back(fb);
        fb += mats[i].nb * G[i];
        L.ready_reserved += (size_t)mats[i].nb * RGMAX;
        L.entries += (size_t)mats[i].nb / 2 * (size_t)G[i];
        any_parts = any_parts || G[i] > 1;
    }
    L.ready_used = (size_t)fb - L.np;
    L.ready_bytes = (sizeof(unsigned int) * (2 * L.ready_reserved + L.np) + 15) / 16 * 16;
    L.zero_bytes = head_bytes + L.ready_bytes;
    // a launch zeroes and uses the regions of the parts it assigns (nb is even: nb * G units per matrix, laid out by the flag
    // bases); a list with more parts than resident workgroups shares workgroups and runs every pair in one part: no exchange
    L.gran_reserved = granules ? 2 * kPlanGranBytes * slots : 0;
    L.gran_used = (granules && any_parts) ? L.ready_used * kPlanGranBytes : 0;
    L.map_off = (kPlanPairBytes * L.np + 255) / 256 * 256;
    L.ent_off = (L.map_off + kPlanMapBytes * L.entries + 255) / 256 * 256;
    L.image_bytes = L.ent_off + kPlanMapBytes * n_ranges;
    L.fits = L.entries <= slots || L.entries == L.np;
    return L;
}

// ---- the three together -----------------------------------------------------------------------------------------------------
struct SweepPlan {
    std::vector<int> G;   // [matrix, work-list order] parts per pair
    PlanShare share;
    SweepLayout layout;
};
inline SweepPlan plan_sweep(const std::vector<PlanMat>& mats, size_t slots, int g_env, size_t head_bytes, bool granules)
{
    SweepPlan p;
    p.G = plan_parts(mats, slots, g_env);
    size_t entries = 0;
    std::vector<int> nb;
    for (size_t i = 0; i < mats.size(); ++i) {
        entries += (size_t)mats[i].nb / 2 * (size_t)p.G[i];
        nb.push_back(mats[i].nb);
    }
    p.share = plan_share(nb, entries, slots);
    p.layout = plan_layout(mats, p.G, slots, head_bytes, granules, p.share.ranges.size());
    return p;
}

} // namespace cyb
