// Weighted Kronecker products into strided tiles: every result block of a fusion-tree outer in ONE launch.
//
// FusionTreeBackend::outer (src/backends/fusion_tree_backend.cpp:2609-2667) is a double loop over the tree-block pairs of a
// times the tree-block pairs of b; each iteration makes block_backend->outer, permute_axes, combine_legs, and then get_item,
// mul, operator+ and set_item per (new codomain tree, new domain tree) into a result that was zero-filled first.  Here an
// *output* record is one destination tile (rows ha * hb, columns wa * wb, inside a coupled block with the leading dimension
// ldd) and a *term* record one contributing (a tree pair, b tree pair) with its coefficient, both read in place:
//   dst[(ra * hb + rb) * ldd + ca * wb + cb] = sum_t c_t * A_t[ra * a_rs + ca * a_cs] * B_t[rb * b_rs + cb * b_cs]
// Every destination element has exactly one owner which adds its terms in ascending order ((c * A) * B, accumulated in
// registers): no float atomics, no zero fill, no second pass, bit-identical from run to run; an output with no terms is
// written as zeros.
//
// The operation is a store stream whose sources are tiny next to the result (as outer_grouped.hip) -- beside a 1 x 1 tile of
// B, as large as it -- so:
//   * the lanes run along the contiguous columns of the destination and every lane stores 16 bytes per step: one complex,
//     or a pair of doubles (cb, cb + 1) where wb is even, ldd is even (or the tile has one row) and dst is 16-byte aligned --
//     a pair then never straddles two values of ca, and every pair of the tile is aligned.  Else one double per lane.
//   * the tile is the 4-level index space (ra, rb, ca, cb) in the flat order of dst (cb counts pairs in pair mode), cut into
//     one-wave work items and walked by a cursor (four digits, destination offset) as wave_items.h describes.  The source
//     offsets are four multiply-adds per term from the digits.
//   * item, record and term are wave-uniform: their fields travel through scalar loads, the term loop is innermost.
#include "wave_items.h"

namespace {

using namespace cyb_items;
typedef cyb_outer_weighted_out Out;
typedef cyb_outer_weighted_term Term;

// one output as the kernel reads it; levels 0..3 = (ra, rb, ca, cb), one stream: the destination (doubles; kC128: complex
// elements)
struct Rec {
    double* dst;
    int64_t first_term, n_terms;
    Levels<4, 1> lv;
    int32_t mode, reserved;
};

typedef cyb_items::Item<4, 1> Item;
typedef cyb_items::Cursor<4, 1> Cursor;

// acc += (c * A) * B of one term at the digits of `c`
template <int MODE> __device__ inline void add_term(typename Val<MODE>::type& acc, const Term& tm, const Cursor& c)
{
    const int64_t oa = (int64_t)c.idx[0] * tm.a_rs + (int64_t)c.idx[2] * tm.a_cs;
    const int64_t ob = (int64_t)c.idx[1] * tm.b_rs + (int64_t)(MODE == kF64x2 ? 2 * c.idx[3] : c.idx[3]) * tm.b_cs;
    const GLOBAL_AS double* a = (const GLOBAL_AS double*)tm.a;
    const GLOBAL_AS double* b = (const GLOBAL_AS double*)tm.b;
    if constexpr (MODE == kF64) {
        acc += (tm.coeff_re * a[oa]) * b[ob];
    } else if constexpr (MODE == kF64x2) {
        const double p = tm.coeff_re * a[oa];
        acc.x += p * b[ob];
        acc.y += p * b[ob + tm.b_cs];
    } else {
        const d2 x = load_c(tm.a, oa, tm.a_real), y = load_c(tm.b, ob, tm.b_real);
        const d2 p = d2{tm.coeff_re * x.x - tm.coeff_im * x.y, tm.coeff_re * x.y + tm.coeff_im * x.x};
        acc.x += p.x * y.x - p.y * y.y;
        acc.y += p.x * y.y + p.y * y.x;
    }
}

template <int MODE> __device__ inline void run_item(const Rec& r, const Item& it, const Term* __restrict__ terms, int lane)
{
    Cursor c;
    start(c, r.lv, it.at, lane, 0);
    double* dst = r.dst;
    for (int64_t k = lane; k < it.count; k += WAVE) {
        typename Val<MODE>::type acc = zero_<MODE>();
        for (int64_t t = r.first_term; t < r.first_term + r.n_terms; ++t) add_term<MODE>(acc, terms[t], c);
        store_<MODE>(dst, c.off[0], acc);
        advance(c, r.lv, r.lv.step, r.lv.step_o, 0);
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) outer_weighted_kernel(const Rec* __restrict__ recs, const Term* __restrict__ terms,
                                                            const Item* __restrict__ items, int n_items)
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

template <bool CPLX>
int outer_weighted(cyb_ctx_t ctx, const Out* outs, int64_t n_outs, const Term* terms, int64_t n_terms, const char* who)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n_outs >= 0 && n_terms >= 0 && (n_outs == 0 || outs) && (n_terms == 0 || terms), "%s: bad lists", who);
    if (n_outs == 0) return CYB_OK;
    std::vector<Term> ht(terms, terms + n_terms);
    for (int64_t t = 0; t < n_terms; ++t) {
        CYB_REQUIRE(CPLX || ht[(size_t)t].coeff_im == 0.0, "%s: term %lld: a complex coefficient at the float64 entry", who, (long long)t);
        if (!CPLX) ht[(size_t)t].a_real = ht[(size_t)t].b_real = 0;
    }
    std::vector<Rec> recs;
    std::vector<int64_t> totals;
    for (int64_t i = 0; i < n_outs; ++i) {
        const Out& o = outs[i];
        CYB_REQUIRE(o.ha >= 0 && o.hb >= 0 && o.wa >= 0 && o.wb >= 0, "%s: output %lld: negative extent", who, (long long)i);
        CYB_REQUIRE_TERM_RANGE(who, i, o, n_terms);
        const int64_t ext[4] = {o.ha, o.hb, o.wa, o.wb};
        int64_t total = 1;
        bool fits = true;
        for (int l = 0; l < 4; ++l) {
            fits = fits && ext[l] <= INT32_MAX / 2 && (ext[l] == 0 || total <= (INT64_MAX >> 4) / ext[l]);
            total = fits ? total * ext[l] : 0;
        }
        CYB_REQUIRE(fits, "%s: output %lld: extent too large", who, (long long)i);
        if (total == 0) continue;
        const int64_t H = o.ha * o.hb, W = o.wa * o.wb;
        CYB_REQUIRE(H == 1 || o.ldd >= W, "%s: output %lld: ldd %lld below the %lld columns of the tile", who, (long long)i, (long long)o.ldd,
                    (long long)W);
        CYB_REQUIRE(o.dst, "%s: output %lld: dst is NULL", who, (long long)i);
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t)
            CYB_REQUIRE(ht[(size_t)t].a && ht[(size_t)t].b, "%s: term %lld: %s is NULL", who, (long long)t, ht[(size_t)t].a ? "b" : "a");
        // pairs of doubles: (cb, cb + 1) share ca, and every pair of every row is 16-byte aligned
        const bool x2 = !CPLX && even_(o.wb) && (H == 1 || even_(o.ldd)) && ((uintptr_t)o.dst & 15) == 0;
        const int64_t V = x2 ? 2 : 1;
        Rec r;
        memset(&r, 0, sizeof(r));
        r.dst = o.dst, r.first_term = o.first_term, r.n_terms = o.n_terms;
        r.mode = CPLX ? kC128 : (x2 ? kF64x2 : kF64);
        int32_t(&e)[4] = r.lv.ext;
        int64_t(&sd)[4] = r.lv.st[0];
        e[0] = (int32_t)o.ha, e[1] = (int32_t)o.hb, e[2] = (int32_t)o.wa, e[3] = (int32_t)(o.wb / V);
        sd[0] = o.hb * o.ldd, sd[1] = o.ldd, sd[2] = o.wb, sd[3] = V;
        set_steps(r.lv, 0);
        recs.push_back(r);
        totals.push_back(total / V);
    }
    std::vector<Item> items;
    cut_items(items, recs, totals);
    return launch_items(ctx, outer_weighted_kernel<CPLX>, recs, ht, items, who);
}

} // namespace

extern "C" {

int cyb_outer_weighted_f64(cyb_ctx_t ctx, const cyb_outer_weighted_out* outs, int64_t n_outs, const cyb_outer_weighted_term* terms, int64_t n_terms)
{
    return outer_weighted<false>(ctx, outs, n_outs, terms, n_terms, "cyb_outer_weighted_f64");
}

int cyb_outer_weighted_c128(cyb_ctx_t ctx, const cyb_outer_weighted_out* outs, int64_t n_outs, const cyb_outer_weighted_term* terms, int64_t n_terms)
{
    return outer_weighted<true>(ctx, outs, n_outs, terms, n_terms, "cyb_outer_weighted_c128");
}

} // extern "C"
