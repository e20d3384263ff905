// Grouped, weighted, strided window copies: every window of every result block of a fusion-tree from_grid / from_tree_pairs
// in ONE launch.
//
// FusionTreeBackend::from_grid (src/backends/fusion_tree_backend.cpp:3375-3518) makes get_item, reshape, copy_block, reshape,
// get_item, operator+, set_item, reshape and set_item per (grid entry, codomain forest, domain forest) into a result that was
// zero-filled first, and scans every block for zeros afterwards; ::from_tree_pairs (:3186-3263) makes permute_axes, reshape and
// set_item per tree pair into zeros.  Here a record is one *window* of a coupled block -- h consecutive rows, nq runs of wn
// consecutive columns, one run every cp columns, inside a block with the leading dimension ldd -- and its source a strided
// view read in place:
//   dst[r * ldd + q * cp + w] = c * src[sum_l r_l * rs[l] + sum_l x_l * cs[l]]          r < h, q < nq, w < wn
// r counted in C order over the row levels rext[], x = q * wn + w in C order over the column levels cext[].  A record without a
// source writes zeros: the cells of a result nothing feeds need no memset.  Every destination element has exactly one owner:
// no atomics, no zero fill, no second pass, bit-identical from run to run; c == 1 stores the bits it loaded.
//
// The operation is a copy stream, so the layout of the work is that of tree_outer.hip:
//   * host: the window is the flat index space u = (r * nq + q) * wn + w, which is the C order of the destination levels
//     (r, q, w) AND of the source levels (r_0 .., x_0 ..).  Source levels of extent 1 are dropped and adjacent levels that
//     continue each other are merged (a contiguous tile of a block: one row level, one column level).  Every record is cut
//     into the one-wave work items of wave_items.h, the lanes of a wave on 64 consecutive units: along a column run where
//     the run is wide, across several runs and rows at once where wn is small -- a stacked leg of multiplicity 1 under a
//     large nq leaves no lane idle.
//   * a lane stores 16 bytes per step: one complex, or a pair of doubles (w, w + 1) where wn is even, cp is even (or nq = 1),
//     ldd is even (or h = 1), dst is 16-byte aligned and the innermost source level has an even extent -- a pair then never
//     straddles two runs or two values of a source level, and every pair of the window is aligned.  Else one double per
//     lane (a window whose runs start 8-byte aligned only is stored 8 bytes wide throughout; the stores of a wave are
//     consecutive either way).  The pair of the source is ONE 16-byte load where its innermost level has stride 1 and every
//     pair is aligned, else two loads.
//   * device: a lane keeps two cursors of wave_items.h (destination: three digits; source: up to twelve) over the same flat
//     units, and an item carries the start of both.
//     Four steps are taken at a time, their loads issued before the first store.
//     The source levels are right-aligned; the unused ones are skipped by wave-uniform branches.
//   * item and record are wave-uniform: their fields travel through scalar loads.
#include "wave_items.h"

namespace {

using namespace cyb_items;
constexpr int ND = 3, NS = 2 * CYB_TREE_PLACE_MAX_LEVELS; // destination levels (r, q, w); source levels at most
constexpr int64_t kMaxExtent = (int64_t)1 << 30;
constexpr int kUnroll = 4; // steps of a lane whose loads are in flight together
typedef cyb_tree_place_rec In;

// one window as the kernel reads it; offsets and strides in doubles (kC128: complex elements of the destination, elements of
// the source's own type).  Source levels s.first .. NS - 1, the innermost last.
struct Rec {
    double* dst;
    const double* src; // NULL: zeros
    double cre, cim;
    Levels<ND, 1> d; // (kF64x2: the last extent counts pairs)
    Levels<NS, 1> s;
    int64_t pair_cs; // kF64x2: distance of the two source elements of a pair
    int32_t mode, src_real, unit, vec_load;
};

struct Item {
    int32_t rec;
    int32_t reserved;
    int64_t count; // flat units of this item
    Start<ND, 1> d; // its first unit
    Start<NS, 1> s;
};

// the value of one unit: c * source, the source's bits under c == 1 (else one product per component pair, no addend), or zeros
template <int MODE> __device__ inline typename Val<MODE>::type load_one(const Rec& r, const double* src, int64_t os, bool zero)
{
    if constexpr (MODE == kF64) {
        if (zero) return 0.0;
        const double v = load_f64(src, os);
        return r.unit ? v : r.cre * v;
    } else if constexpr (MODE == kF64x2) {
        if (zero) return d2{0.0, 0.0};
        const d2 v = r.vec_load ? load_x2(src, os) : d2{load_f64(src, os), load_f64(src, os + r.pair_cs)};
        return r.unit ? v : d2{r.cre * v.x, r.cre * v.y};
    } else {
        if (zero) return d2{0.0, 0.0};
        if (r.src_real) {
            const double x = load_f64(src, os);
            return r.unit ? d2{x, 0.0} : d2{r.cre * x, r.cim * x};
        }
        const d2 x = load_c(src, os, false);
        return r.unit ? x : d2{r.cre * x.x - r.cim * x.y, r.cre * x.y + r.cim * x.x};
    }
}

template <int MODE> __device__ inline void run_item(const Rec& r, const Item& it, int lane)
{
    const bool zero = r.src == nullptr; // wave-uniform, as every field of the record
    const int s_first = zero ? NS : r.s.first;
    Cursor<ND, 1> cd;
    Cursor<NS, 1> cs;
    start(cd, r.d, it.d, lane, 0);
    start(cs, r.s, it.s, lane, s_first);
    double* dst = r.dst;
    const double* src = r.src;
    // kUnroll steps at a time: their loads are issued before the first store, so that a lane has several requests in flight
    // (destination and source may alias as far as the compiler knows; it would not move a load above a store)
    for (int64_t k = lane; k < it.count; k += kUnroll * WAVE) {
        typename Val<MODE>::type v[kUnroll];
        int64_t at[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            at[u] = cd.off[0];
            if (k + u * WAVE < it.count) v[u] = load_one<MODE>(r, src, cs.off[0], zero);
            advance(cd, r.d, r.d.step, r.d.step_o, 0);
            advance(cs, r.s, r.s.step, r.s.step_o, s_first);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (k + u * WAVE < it.count) store_<MODE>(dst, at[u], v[u]);
    }
}

template <bool CPLX> __global__ void __launch_bounds__(NT) tree_place_kernel(const Rec* __restrict__ recs, const Item* __restrict__ items, int n_items)
{
    int i, lane;
    if (!my_item(i, lane, n_items)) return;
    const Item& it = items[i];
    const Rec& r = recs[it.rec];
    if constexpr (CPLX) {
        run_item<kC128>(r, it, lane);
    } else {
        if (r.mode == kF64x2)
            run_item<kF64x2>(r, it, lane);
        else
            run_item<kF64>(r, it, lane);
    }
}

// validates the list and turns it into the records and work items of the launch (both empty: nothing to do)
template <bool CPLX> int plan_place(std::vector<Rec>& recs, std::vector<Item>& items, const In* in, int64_t n_recs, const char* who)
{
    std::vector<int64_t> totals;
    for (int64_t i = 0; i < n_recs; ++i) {
        const In& o = in[i];
        const long long ii = (long long)i;
        CYB_REQUIRE(o.n_row_levels >= 0 && o.n_row_levels <= CYB_TREE_PLACE_MAX_LEVELS && o.n_col_levels >= 0 && o.n_col_levels <= CYB_TREE_PLACE_MAX_LEVELS,
                    "%s: record %lld: %d row levels and %d column levels, at most %d each", who, ii, (int)o.n_row_levels, (int)o.n_col_levels,
                    CYB_TREE_PLACE_MAX_LEVELS);
        bool neg = o.h < 0 || o.nq < 0 || o.wn < 0, big = o.h > kMaxExtent || o.nq > kMaxExtent || o.wn > kMaxExtent;
        for (int l = 0; l < o.n_row_levels; ++l) neg = neg || o.rext[l] < 0, big = big || o.rext[l] > kMaxExtent;
        for (int l = 0; l < o.n_col_levels; ++l) neg = neg || o.cext[l] < 0, big = big || o.cext[l] > kMaxExtent;
        CYB_REQUIRE(!neg, "%s: record %lld: negative extent", who, ii);
        CYB_REQUIRE(!big, "%s: record %lld: extent too large", who, ii);
        CYB_REQUIRE(CPLX || o.coeff_im == 0.0, "%s: record %lld: a complex coefficient at the float64 entry", who, ii);
        if (o.src) { // (a record of zeros has no index space to agree with)
            CYB_REQUIRE(product_is(o.rext, o.n_row_levels, o.h), "%s: record %lld: the row levels do not multiply to h = %lld", who, ii, (long long)o.h);
            CYB_REQUIRE(product_is(o.cext, o.n_col_levels, o.nq * o.wn), "%s: record %lld: the column levels do not multiply to nq * wn = %lld", who, ii,
                        (long long)(o.nq * o.wn));
        }
        if (o.h == 0 || o.nq == 0 || o.wn == 0) continue;
        CYB_REQUIRE((__int128)o.h * o.nq * o.wn <= (__int128)(INT64_MAX >> 4), "%s: record %lld: extent too large", who, ii);
        CYB_REQUIRE(o.nq == 1 || o.cp >= o.wn, "%s: record %lld: cp %lld below the %lld columns of a run", who, ii, (long long)o.cp, (long long)o.wn);
        CYB_REQUIRE(o.h == 1 || (__int128)o.ldd >= (__int128)(o.nq - 1) * (o.nq > 1 ? o.cp : 0) + o.wn,
                    "%s: record %lld: ldd %lld below the columns the window spans", who, ii, (long long)o.ldd);
        CYB_REQUIRE(o.dst, "%s: record %lld: dst is NULL", who, ii);
        const int64_t cp = o.nq > 1 ? o.cp : o.wn, ldd = o.h > 1 ? o.ldd : 0;
        // the source levels: extent 1 dropped, a level that continues its inner neighbour merged into it
        int64_t le[NS], ls[NS];
        int n = 0;
        if (o.src) {
            for (int l = 0; l < o.n_row_levels + o.n_col_levels; ++l, ++n) {
                le[n] = l < o.n_row_levels ? o.rext[l] : o.cext[l - o.n_row_levels];
                ls[n] = l < o.n_row_levels ? o.rs[l] : o.cs[l - o.n_row_levels];
            }
            n = merge_levels(le, ls, n, kMaxExtent);
        }
        // pairs of doubles: (w, w + 1) share q and every source digit but the innermost, and every pair is 16-byte aligned
        bool x2 = !CPLX && even_(o.wn) && even_(cp) && even_(ldd) && ((uintptr_t)o.dst & 15) == 0;
        if (x2 && o.src) x2 = n > 0 && even_(le[n - 1]);
        const int64_t V = x2 ? 2 : 1;
        Rec r;
        memset(&r, 0, sizeof(r));
        r.dst = o.dst, r.src = o.src;
        r.cre = o.coeff_re, r.cim = CPLX ? o.coeff_im : 0.0;
        r.unit = r.cre == 1.0 && r.cim == 0.0;
        r.src_real = CPLX && o.src_real != 0;
        r.mode = CPLX ? kC128 : (x2 ? kF64x2 : kF64);
        r.d.ext[0] = (int32_t)o.h, r.d.ext[1] = (int32_t)o.nq, r.d.ext[2] = (int32_t)(o.wn / V);
        r.d.st[0][0] = ldd, r.d.st[0][1] = cp, r.d.st[0][2] = V;
        set_steps(r.d, 0);
        const int s_first = NS - n;
        for (int l = 0; l < n; ++l) r.s.ext[s_first + l] = (int32_t)le[l], r.s.st[0][s_first + l] = ls[l];
        if (x2 && o.src) {
            r.pair_cs = ls[n - 1];
            r.s.ext[NS - 1] = (int32_t)(le[n - 1] / 2), r.s.st[0][NS - 1] = 2 * ls[n - 1];
            r.vec_load = ls[n - 1] == 1 && ((uintptr_t)o.src & 15) == 0;
            for (int l = 0; l + 1 < n; ++l) r.vec_load = r.vec_load && even_(ls[l]);
        }
        set_steps(r.s, s_first);
        recs.push_back(r);
        totals.push_back(o.h * o.nq * (o.wn / V));
    }
    // both cursors of an item start at the same flat unit
    const int64_t chunk = chunk_for(totals);
    for (size_t i = 0; i < recs.size(); ++i)
        for (int64_t e0 = 0; e0 < totals[i]; e0 += chunk)
            items.push_back(Item{(int32_t)i, 0, std::min(chunk, totals[i] - e0), start_at(recs[i].d, e0), start_at(recs[i].s, e0)});
    CYB_REQUIRE(items.size() < ((size_t)1 << 31), "%s: too many work items", who);
    return CYB_OK;
}

template <bool CPLX> int tree_place(cyb_ctx_t ctx, const In* in, int64_t n_recs, const char* who)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n_recs >= 0 && (n_recs == 0 || in), "%s: bad list", who);
    std::vector<Rec> recs;
    std::vector<Item> items;
    CYB_TRY(plan_place<CPLX>(recs, items, in, n_recs, who));
    return cyb_flat::launch<ITEMS_PER_GROUP>(ctx, who, tree_place_kernel<CPLX>, cyb_flat::arrays(recs, items), (int)items.size());
}

} // namespace

extern "C" {

int cyb_tree_place_f64(cyb_ctx_t ctx, const cyb_tree_place_rec* recs, int64_t n_recs) { return tree_place<false>(ctx, recs, n_recs, "cyb_tree_place_f64"); }

int cyb_tree_place_c128(cyb_ctx_t ctx, const cyb_tree_place_rec* recs, int64_t n_recs) { return tree_place<true>(ctx, recs, n_recs, "cyb_tree_place_c128"); }

} // extern "C"
