// Weighted sums of strided windows: every strip of every result block of a factorized fusion-tree move in ONE launch per side.
//
// FactorizedTreeMapping::transform_splitting_trees / ::transform_fusion_trees (src/backends/fusion_tree_mapping.cpp:627-674,
// :676-725) make get_item, mul and operator+ per (new tree, old tree), then permute_combined_idx and set_item per new tree,
// into a block that was zero-filled first.  Here an *output* record is one window of a result block, the window of
// tree_place.hip -- h consecutive rows, nq runs of wn consecutive columns, one run every cp columns, leading dimension ldd --
// with ONE table of source levels, and a *term* record one old tree that feeds it: its block, its coefficient and where its
// rows (or columns) begin.  The terms of a strip differ in the old tree they read, never in the permutation:
//   dst[r * ldd + q * cp + w] = sum_t c_t * src_t[base_t + sum_l r_l * rs[l] + sum_l x_l * cs[l]]          r < h, q < nq, w < wn
// r counted in C order over the row levels rext[], x = q * wn + w in C order over the column levels cext[].  Every
// destination element has exactly one owner which adds its terms in ascending order in registers: no atomics, no zero fill, no
// second pass, bit-identical from run to run; an output with no terms is written as zeros; the first term is assigned, not
// added to a zero, so one term with c == 1 stores the bits it loaded.
//
// tree_place.hip is this operation with exactly one source per record, and the layout of the work is its layout:
//   * host: the window is the flat index space u = (r * nq + q) * wn + w, the C order of the destination levels (r, q, w) AND
//     of the source levels.  Source levels of extent 1 are dropped, levels that continue their inner neighbour merged
//     (merge_levels); every record is cut into the one-wave work items of wave_items.h.
//   * a lane stores 16 bytes per step: one complex, or a pair of doubles (w, w + 1) under the conditions of tree_place.hip (wn,
//     cp, ldd even, dst 16-byte aligned, the innermost source level of even extent).  The pair of a source is ONE 16-byte
//     load where the innermost source level has the stride 1 and every pair of EVERY term of the record is aligned, else two
//     loads.  A record whose innermost source level is not the innermost destination level (a permutation that moves the
//     last multiplicity of a column pass) has no stride-1 level there: its loads are gathered 8 (16: complex) bytes at a time.
//   * device: a lane keeps two cursors (destination: three digits; source: up to twelve) over the same flat units.  Four
//     steps are taken at a time; for every term their loads are issued together, and all loads before the first store.
//   * item, record and term are wave-uniform: their fields travel through scalar loads.
#include "wave_items.h"

namespace {

using namespace cyb_items;
constexpr int ND = 3, NS = 2 * CYB_TREE_PLACE_MAX_LEVELS; // destination levels (r, q, w); source levels at most
constexpr int64_t kMaxExtent = (int64_t)1 << 30;
constexpr int kUnroll = 4; // steps of a lane whose loads are in flight together
typedef cyb_tree_strip_out Out;
typedef cyb_tree_strip_term InTerm;

// one output as the kernel reads it; offsets and strides in doubles (kC128: complex elements of the destination, elements of
// a source's own type).  Source levels s.first .. NS - 1, the innermost last.
struct Rec {
    double* dst;
    int64_t first_term, n_terms;
    Levels<ND, 1> d; // (kF64x2: the last extent counts pairs)
    Levels<NS, 1> s;
    int64_t pair_cs; // kF64x2: distance of the two source elements of a pair
    int32_t mode, vec_load;
};

// one term as the kernel reads it: src addresses the element at the term's base offset
struct Term {
    const double* src;
    double cre, cim;
    int32_t unit, src_real;
};

struct Item {
    int32_t rec;
    int32_t reserved;
    int64_t count; // flat units of this item
    Start<ND, 1> d; // its first unit
    Start<NS, 1> s;
};

// c * source of one unit: the source's bits under c == 1, else one product per component pair
template <int MODE> __device__ inline typename Val<MODE>::type term_value(const Rec& r, const Term& tm, int64_t os)
{
    if constexpr (MODE == kF64) {
        const double v = load_f64(tm.src, os);
        return tm.unit ? v : tm.cre * v;
    } else if constexpr (MODE == kF64x2) {
        const d2 v = r.vec_load ? load_x2(tm.src, os) : d2{load_f64(tm.src, os), load_f64(tm.src, os + r.pair_cs)};
        return tm.unit ? v : d2{tm.cre * v.x, tm.cre * v.y};
    } else {
        if (tm.src_real) {
            const double x = load_f64(tm.src, os);
            return tm.unit ? d2{x, 0.0} : d2{tm.cre * x, tm.cim * x};
        }
        const d2 x = load_c(tm.src, os, false);
        return tm.unit ? x : d2{tm.cre * x.x - tm.cim * x.y, tm.cre * x.y + tm.cim * x.x};
    }
}

template <int MODE> __device__ inline void run_item(const Rec& r, const Item& it, const Term* __restrict__ terms, int lane)
{
    const int64_t t0 = r.first_term, t1 = t0 + r.n_terms; // wave-uniform, as every field of the record
    const int s_first = t0 < t1 ? r.s.first : NS;
    Cursor<ND, 1> cd;
    Cursor<NS, 1> cs;
    start(cd, r.d, it.d, lane, 0);
    start(cs, r.s, it.s, lane, s_first);
    double* dst = r.dst;
    // kUnroll steps at a time: the loads of a term are issued together, all of them before the first store (destination and
    // sources may alias as far as the compiler knows; it would not move a load above a store)
    for (int64_t k = lane; k < it.count; k += kUnroll * WAVE) {
        typename Val<MODE>::type v[kUnroll];
        int64_t at[kUnroll], os[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            at[u] = cd.off[0], os[u] = cs.off[0];
            v[u] = zero_<MODE>();
            advance(cd, r.d, r.d.step, r.d.step_o, 0);
            advance(cs, r.s, r.s.step, r.s.step_o, s_first);
        }
        if (t0 < t1) { // the first term is assigned: no sum with a zero that would turn -0.0 into 0.0
            const Term& tm = terms[t0];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (k + u * WAVE < it.count) v[u] = term_value<MODE>(r, tm, os[u]);
        }
        for (int64_t t = t0 + 1; t < t1; ++t) {
            const Term& tm = terms[t];
            typename Val<MODE>::type x[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (k + u * WAVE < it.count) x[u] = term_value<MODE>(r, tm, os[u]);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
                if (k + u * WAVE < it.count) v[u] += x[u];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (k + u * WAVE < it.count) store_<MODE>(dst, at[u], v[u]);
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) tree_strip_kernel(const Rec* __restrict__ recs, const Term* __restrict__ terms, const Item* __restrict__ items,
                                                        int n_items)
{
    int i, lane;
    if (!my_item(i, lane, n_items)) return;
    const Item& it = items[i];
    const Rec& r = recs[it.rec];
    if constexpr (CPLX) {
        run_item<kC128>(r, it, terms, lane);
    } else {
        if (r.mode == kF64x2)
            run_item<kF64x2>(r, it, terms, lane);
        else
            run_item<kF64>(r, it, terms, lane);
    }
}

// validates the lists and turns them into the records, terms and work items of the launch (no items: nothing to do)
template <bool CPLX>
int plan_strip(std::vector<Rec>& recs, std::vector<Term>& terms, std::vector<Item>& items, const Out* outs, int64_t n_outs, const InTerm* in_terms,
               int64_t n_terms, const char* who)
{
    terms.resize((size_t)n_terms);
    for (int64_t t = 0; t < n_terms; ++t) {
        const InTerm& tm = in_terms[t];
        CYB_REQUIRE(CPLX || tm.coeff_im == 0.0, "%s: term %lld: a complex coefficient at the float64 entry", who, (long long)t);
        Term& k = terms[(size_t)t];
        k.src_real = CPLX && tm.src_real != 0;
        k.src = tm.src ? tm.src + tm.base * (CPLX && !k.src_real ? 2 : 1) : nullptr;
        k.cre = tm.coeff_re, k.cim = CPLX ? tm.coeff_im : 0.0;
        k.unit = k.cre == 1.0 && k.cim == 0.0;
    }
    std::vector<int64_t> totals;
    for (int64_t i = 0; i < n_outs; ++i) {
        const Out& o = outs[i];
        const long long ii = (long long)i;
        CYB_REQUIRE(o.n_row_levels >= 0 && o.n_row_levels <= CYB_TREE_PLACE_MAX_LEVELS && o.n_col_levels >= 0 && o.n_col_levels <= CYB_TREE_PLACE_MAX_LEVELS,
                    "%s: output %lld: %d row levels and %d column levels, at most %d each", who, ii, (int)o.n_row_levels, (int)o.n_col_levels,
                    CYB_TREE_PLACE_MAX_LEVELS);
        CYB_REQUIRE_TERM_RANGE(who, i, o, n_terms);
        bool neg = o.h < 0 || o.nq < 0 || o.wn < 0, big = o.h > kMaxExtent || o.nq > kMaxExtent || o.wn > kMaxExtent;
        for (int l = 0; l < o.n_row_levels; ++l) neg = neg || o.rext[l] < 0, big = big || o.rext[l] > kMaxExtent;
        for (int l = 0; l < o.n_col_levels; ++l) neg = neg || o.cext[l] < 0, big = big || o.cext[l] > kMaxExtent;
        CYB_REQUIRE(!neg, "%s: output %lld: negative extent", who, ii);
        CYB_REQUIRE(!big, "%s: output %lld: extent too large", who, ii);
        const bool fed = o.n_terms > 0; // (an output of zeros has no index space to agree with)
        if (fed) {
            CYB_REQUIRE(product_is(o.rext, o.n_row_levels, o.h), "%s: output %lld: the row levels do not multiply to h = %lld", who, ii, (long long)o.h);
            CYB_REQUIRE(product_is(o.cext, o.n_col_levels, o.nq * o.wn), "%s: output %lld: the column levels do not multiply to nq * wn = %lld", who, ii,
                        (long long)(o.nq * o.wn));
        }
        if (o.h == 0 || o.nq == 0 || o.wn == 0) continue;
        CYB_REQUIRE((__int128)o.h * o.nq * o.wn <= (__int128)(INT64_MAX >> 4), "%s: output %lld: extent too large", who, ii);
        CYB_REQUIRE(o.nq == 1 || o.cp >= o.wn, "%s: output %lld: cp %lld below the %lld columns of a run", who, ii, (long long)o.cp, (long long)o.wn);
        CYB_REQUIRE(o.h == 1 || (__int128)o.ldd >= (__int128)(o.nq - 1) * (o.nq > 1 ? o.cp : 0) + o.wn,
                    "%s: output %lld: ldd %lld below the columns the window spans", who, ii, (long long)o.ldd);
        CYB_REQUIRE(o.dst, "%s: output %lld: dst is NULL", who, ii);
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t)
            CYB_REQUIRE(in_terms[t].src, "%s: term %lld: src is NULL", who, (long long)t);
        const int64_t cp = o.nq > 1 ? o.cp : o.wn, ldd = o.h > 1 ? o.ldd : 0;
        int64_t le[NS], ls[NS];
        int n = 0;
        if (fed) {
            for (int l = 0; l < o.n_row_levels + o.n_col_levels; ++l, ++n) {
                le[n] = l < o.n_row_levels ? o.rext[l] : o.cext[l - o.n_row_levels];
                ls[n] = l < o.n_row_levels ? o.rs[l] : o.cs[l - o.n_row_levels];
            }
            n = merge_levels(le, ls, n, kMaxExtent);
        }
        // pairs of doubles: (w, w + 1) share q and every source digit but the innermost, and every pair is 16-byte aligned
        bool x2 = !CPLX && even_(o.wn) && even_(cp) && even_(ldd) && ((uintptr_t)o.dst & 15) == 0;
        if (x2 && fed) x2 = n > 0 && even_(le[n - 1]);
        const int64_t V = x2 ? 2 : 1;
        Rec r;
        memset(&r, 0, sizeof(r));
        r.dst = o.dst, r.first_term = o.first_term, r.n_terms = o.n_terms;
        r.mode = CPLX ? kC128 : (x2 ? kF64x2 : kF64);
        r.d.ext[0] = (int32_t)o.h, r.d.ext[1] = (int32_t)o.nq, r.d.ext[2] = (int32_t)(o.wn / V);
        r.d.st[0][0] = ldd, r.d.st[0][1] = cp, r.d.st[0][2] = V;
        set_steps(r.d, 0);
        const int s_first = NS - n;
        for (int l = 0; l < n; ++l) r.s.ext[s_first + l] = (int32_t)le[l], r.s.st[0][s_first + l] = ls[l];
        if (x2 && fed) {
            r.pair_cs = ls[n - 1];
            r.s.ext[NS - 1] = (int32_t)(le[n - 1] / 2), r.s.st[0][NS - 1] = 2 * ls[n - 1];
            r.vec_load = ls[n - 1] == 1;
            for (int l = 0; l + 1 < n; ++l) r.vec_load = r.vec_load && even_(ls[l]);
            for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t) r.vec_load = r.vec_load && ((uintptr_t)terms[(size_t)t].src & 15) == 0;
        }
        set_steps(r.s, s_first);
        recs.push_back(r);
        totals.push_back(o.h * o.nq * (o.wn / V));
    }
    // both cursors of an item start at the same flat unit
    const int64_t chunk = chunk_for(totals);
    size_t n_items = 0;
    for (int64_t t : totals) n_items += (size_t)((t + chunk - 1) / chunk);
    CYB_REQUIRE(n_items < ((size_t)1 << 31), "%s: too many work items", who);
    items.reserve(n_items); // (a large strip is thousands of items: no regrowth while they are cut)
    for (size_t i = 0; i < recs.size(); ++i) {
        // the start of the next item is this one's advanced by `chunk` units: the cursor's additions instead of a division per
        // level and item (a record of one item never advances: its chunk may reach beyond the table)
        const Rec& r = recs[i];
        const bool more = totals[i] > chunk;
        const Start<ND, 1> dd = more ? start_at(r.d, chunk) : Start<ND, 1>{};
        const Start<NS, 1> ds = more ? start_at(r.s, chunk) : Start<NS, 1>{};
        Cursor<ND, 1> cd = {};
        Cursor<NS, 1> cs = {};
        for (int64_t e0 = 0; e0 < totals[i]; e0 += chunk) {
            Item it = {(int32_t)i, 0, std::min(chunk, totals[i] - e0), {}, {}};
            it.d.off[0] = cd.off[0], it.s.off[0] = cs.off[0];
            memcpy(it.d.idx, cd.idx, sizeof(cd.idx));
            memcpy(it.s.idx, cs.idx, sizeof(cs.idx));
            items.push_back(it);
            if (e0 + chunk < totals[i]) {
                advance(cd, r.d, dd.idx, dd.off, 0);
                advance(cs, r.s, ds.idx, ds.off, r.s.first);
            }
        }
    }
    return CYB_OK;
}

template <bool CPLX> int tree_strip(cyb_ctx_t ctx, const Out* outs, int64_t n_outs, const InTerm* in_terms, int64_t n_terms, const char* who)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n_outs >= 0 && n_terms >= 0 && (n_outs == 0 || outs) && (n_terms == 0 || in_terms), "%s: bad lists", who);
    std::vector<Rec> recs;
    std::vector<Term> terms;
    std::vector<Item> items;
    CYB_TRY(plan_strip<CPLX>(recs, terms, items, outs, n_outs, in_terms, n_terms, who));
    return launch_items(ctx, tree_strip_kernel<CPLX>, recs, terms, items, who);
}

} // namespace

extern "C" {

int cyb_tree_strip_f64(cyb_ctx_t ctx, const cyb_tree_strip_out* outs, int64_t n_outs, const cyb_tree_strip_term* terms, int64_t n_terms)
{
    return tree_strip<false>(ctx, outs, n_outs, terms, n_terms, "cyb_tree_strip_f64");
}

int cyb_tree_strip_c128(cyb_ctx_t ctx, const cyb_tree_strip_out* outs, int64_t n_outs, const cyb_tree_strip_term* terms, int64_t n_terms)
{
    return tree_strip<true>(ctx, outs, n_outs, terms, n_terms, "cyb_tree_strip_c128");
}

} // extern "C"
