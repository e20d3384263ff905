// Weighted short contractions into strided tiles: every result block of a fusion-tree partial_compose in ONE launch.
//
// FusionTreeBackend::partial_compose (src/backends/fusion_tree_backend.cpp:2670-2880) is a five-deep loop -- outer ("dummy")
// trees, b's codomain trees, b's domain trees, old trees and new trees of insert_at -- and every innermost iteration makes
// get_item, reshape, tdot, permute_axes, reshape, as_scalar, get_item, mul, operator+ and set_item into a result that was
// zero-filled first.  Here an *output* record is one destination tile seen as the 4-level index space (x0, x1, x2, x3) in C
// order with explicit destination strides sd[4]; one level, axis in {1, 2}, carries the surviving index n of b.  A *term*
// record is one contributing (old tree, b tree pair) with its coefficient, its own contracted extent K, the strides sa[4] of
// A (sa[axis]: the stride of the contracted index k) and the strides b_ns, b_ks of B, all read in place:
//   dst[sum_l x_l sd[l]] = sum_t c_t * sum_{k < K_t} A_t[sum_{l != axis} x_l sa[l] + k sa[axis]] * B_t[x_axis b_ns + k b_ks]
// Every destination element has exactly one owner: within a term it sums k ascending in registers, then adds c_t * that sum,
// terms ascending: no float atomics, no zero fill, no second pass, bit-identical from run to run; an output with no terms is
// written as zeros, a term with K = 0 adds nothing.
//
// K and the extent of level `axis` are the multiplicities of physical / MPO legs (1 to a few dozen): the contraction is a
// short register loop per lane and the operation is a stream over A and the result (no MFMA; B tiles are tiny and reread
// through the cache, no LDS).  The layout of the work is that of tree_outer.hip:
//   * the lanes run along the flat (C) order of the four levels and every lane stores 16 bytes per step where it can: one
//     complex, or a pair of doubles.  PAIRING RULE (float64 entry): let p be the last level whose extent is above 1 -- the
//     level the flat order walks fastest; in the domain layout with m2 = 1 that is n, not x3.  A record runs on pairs
//     (x_p, x_p + 1) iff sd[p] == 1, ext[p] is even, sd[l] is even for every level l < p whose extent is above 1, and dst is
//     16-byte aligned: every pair of the tile is then aligned and never straddles two values of an outer level.  Else one
//     double per lane.  With p == axis the two elements of a pair share A and differ in B (by b_ns); else they share B and
//     differ in A (by sa[p]).
//   * WHERE n RUNS (every entry): iff p != axis -- n is not the level the flat order walks fastest -- n leaves the flat order
//     and runs in the registers of a lane, kNB values at a time: a unit is then one (x_l, l != axis), a lane loads A once
//     per k for kNB results, the B addresses are wave-uniform, and the lane stores its kNB results sd[axis] apart (along p
//     the stores of the wave stay contiguous).  With p == axis (the domain layout with m2 = 1, a codomain tile of one
//     column) n stays in the lanes, which keeps those stores contiguous.  The order of the sums of an element is the same.
//   * every record is cut into one-wave work items and walked by a cursor (four digits, destination offset) as
//     wave_items.h describes.  The source offsets are four multiply-adds per term from the digits.
//   * item, record and term are wave-uniform: their fields travel through scalar loads; the k loop is innermost.
#include "wave_items.h"

namespace {

using namespace cyb_items;
constexpr int64_t kMaxExtent = (int64_t)1 << 30;
constexpr int kNB = 4; // values of n a lane holds in registers at a time
typedef cyb_compose_weighted_out Out;
typedef cyb_compose_weighted_term Term;

// one output as the kernel reads it; one stream: the destination (doubles; kC128: complex elements)
struct Rec {
    double* dst;
    int64_t first_term, n_terms;
    Levels<4, 1> lv;                    // (kF64x2: ext[pair] counts pairs)
    int32_t mode, axis, pair;           // pair: the level that counts pairs (kF64x2), else -1
    int32_t n_reg;                      // n in registers: its extent N (ext[axis] is 1 then); 0: n runs in the lanes
    int64_t sn;                         // destination stride of n (as the stream)
};

typedef cyb_items::Item<4, 1> Item;
typedef cyb_items::Cursor<4, 1> Cursor;

// acc += c * sum_k A[k] * B[k] of one term at the digits of `c`
template <int MODE> __device__ inline void add_term(typename Val<MODE>::type& acc, const Term& tm, const Rec& r, const Cursor& c)
{
    int64_t oa = 0, ob = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int64_t x = (MODE == kF64x2 && l == r.pair) ? 2 * (int64_t)c.idx[l] : (int64_t)c.idx[l];
        oa += l == r.axis ? 0 : x * tm.sa[l];
        ob += l == r.axis ? x * tm.b_ns : 0;
    }
    const int64_t ka = tm.sa[r.axis], kb = tm.b_ks;
    const GLOBAL_AS double* a = (const GLOBAL_AS double*)tm.a;
    const GLOBAL_AS double* b = (const GLOBAL_AS double*)tm.b;
    if constexpr (MODE == kF64) {
        double s = 0.0;
        for (int64_t k = 0; k < tm.K; ++k) s += a[oa + k * ka] * b[ob + k * kb];
        acc += tm.coeff_re * s;
    } else if constexpr (MODE == kF64x2) {
        // the second element of the pair: the next n (it shares A), or the next index of another level (it shares B)
        const int64_t pa = r.pair == r.axis ? 0 : tm.sa[r.pair & 3];
        const int64_t pb = r.pair == r.axis ? tm.b_ns : 0;
        double s0 = 0.0, s1 = 0.0;
        for (int64_t k = 0; k < tm.K; ++k) {
            s0 += a[oa + k * ka] * b[ob + k * kb];
            s1 += a[oa + pa + k * ka] * b[ob + pb + k * kb];
        }
        acc.x += tm.coeff_re * s0;
        acc.y += tm.coeff_re * s1;
    } else {
        d2 s = d2{0.0, 0.0};
        for (int64_t k = 0; k < tm.K; ++k) {
            const int64_t ia = oa + k * ka, ib = ob + k * kb;
            const d2 x = load_c(tm.a, ia, tm.a_real), y = load_c(tm.b, ib, tm.b_real);
            s.x += x.x * y.x - x.y * y.y;
            s.y += x.x * y.y + x.y * y.x;
        }
        acc.x += tm.coeff_re * s.x - tm.coeff_im * s.y;
        acc.y += tm.coeff_re * s.y + tm.coeff_im * s.x;
    }
}

// acc[j] += c * sum_k A[k] * B_{n0 + j}[k], j < nn <= kNB, of one term at the digits of `c` (whose digit of `axis` is 0)
template <int MODE>
__device__ inline void add_term_block(typename Val<MODE>::type (&acc)[kNB], const Term& tm, const Rec& r, const Cursor& c, int32_t n0, int32_t nn)
{
    int64_t oa = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int64_t x = (MODE == kF64x2 && l == r.pair) ? 2 * (int64_t)c.idx[l] : (int64_t)c.idx[l];
        oa += l == r.axis ? 0 : x * tm.sa[l];
    }
    const int64_t ka = tm.sa[r.axis], kb = tm.b_ks, ob = (int64_t)n0 * tm.b_ns;
    const GLOBAL_AS double* a = (const GLOBAL_AS double*)tm.a;
    const GLOBAL_AS double* b = (const GLOBAL_AS double*)tm.b;
    if constexpr (MODE == kF64) {
        double s[kNB] = {};
        for (int64_t k = 0; k < tm.K; ++k) {
            const double x = a[oa + k * ka];
#pragma unroll
            for (int j = 0; j < kNB; ++j)
                if (j < nn) s[j] += x * b[ob + j * tm.b_ns + k * kb];
        }
#pragma unroll
        for (int j = 0; j < kNB; ++j) acc[j] += tm.coeff_re * s[j];
    } else if constexpr (MODE == kF64x2) {
        const int64_t pa = tm.sa[r.pair & 3]; // (pair != axis here)
        d2 s[kNB] = {};
        for (int64_t k = 0; k < tm.K; ++k) {
            const double x0 = a[oa + k * ka], x1 = a[oa + pa + k * ka];
#pragma unroll
            for (int j = 0; j < kNB; ++j)
                if (j < nn) {
                    const double y = b[ob + j * tm.b_ns + k * kb];
                    s[j].x += x0 * y;
                    s[j].y += x1 * y;
                }
        }
#pragma unroll
        for (int j = 0; j < kNB; ++j) {
            acc[j].x += tm.coeff_re * s[j].x;
            acc[j].y += tm.coeff_re * s[j].y;
        }
    } else {
        d2 s[kNB] = {};
        for (int64_t k = 0; k < tm.K; ++k) {
            const int64_t ia = oa + k * ka;
            const d2 x = load_c(tm.a, ia, tm.a_real);
#pragma unroll
            for (int j = 0; j < kNB; ++j)
                if (j < nn) {
                    const int64_t ib = ob + j * tm.b_ns + k * kb;
                    const d2 y = load_c(tm.b, ib, tm.b_real);
                    s[j].x += x.x * y.x - x.y * y.y;
                    s[j].y += x.x * y.y + x.y * y.x;
                }
        }
#pragma unroll
        for (int j = 0; j < kNB; ++j) {
            acc[j].x += tm.coeff_re * s[j].x - tm.coeff_im * s[j].y;
            acc[j].y += tm.coeff_re * s[j].y + tm.coeff_im * s[j].x;
        }
    }
}

template <int MODE, bool NREG> __device__ inline void run_item(const Rec& r, const Item& it, const Term* __restrict__ terms, int lane)
{
    typedef typename Val<MODE>::type T;
    Cursor c;
    start(c, r.lv, it.at, lane, 0);
    double* dst = r.dst;
    for (int64_t u = lane; u < it.count; u += WAVE) {
        if constexpr (NREG) {
            for (int32_t n0 = 0; n0 < r.n_reg; n0 += kNB) {
                const int32_t nn = r.n_reg - n0 < kNB ? r.n_reg - n0 : kNB;
                T acc[kNB] = {};
                for (int64_t t = r.first_term; t < r.first_term + r.n_terms; ++t) add_term_block<MODE>(acc, terms[t], r, c, n0, nn);
#pragma unroll
                for (int j = 0; j < kNB; ++j)
                    if (j < nn) store_<MODE>(dst, c.off[0] + (int64_t)(n0 + j) * r.sn, acc[j]);
            }
        } else {
            T acc = zero_<MODE>();
            for (int64_t t = r.first_term; t < r.first_term + r.n_terms; ++t) add_term<MODE>(acc, terms[t], r, c);
            store_<MODE>(dst, c.off[0], acc);
        }
        advance(c, r.lv, r.lv.step, r.lv.step_o, 0);
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) compose_weighted_kernel(const Rec* __restrict__ recs, const Term* __restrict__ terms,
                                                              const Item* __restrict__ items, int n_items)
{
    int i, lane;
    if (!my_item(i, lane, n_items)) return;
    const Item& it = items[i];
    const Rec& r = recs[it.rec];
    if (r.n_reg) {
        if constexpr (CPLX)
            run_item<kC128, true>(r, it, terms, lane);
        else if (r.mode == kF64x2)
            run_item<kF64x2, true>(r, it, terms, lane);
        else
            run_item<kF64, true>(r, it, terms, lane);
    } else {
        if constexpr (CPLX)
            run_item<kC128, false>(r, it, terms, lane);
        else if (r.mode == kF64x2)
            run_item<kF64x2, false>(r, it, terms, lane);
        else
            run_item<kF64, false>(r, it, terms, lane);
    }
}

template <bool CPLX>
int compose_weighted(cyb_ctx_t ctx, const Out* outs, int64_t n_outs, const Term* terms, int64_t n_terms, const char* who)
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
        CYB_REQUIRE(o.ext[0] >= 0 && o.ext[1] >= 0 && o.ext[2] >= 0 && o.ext[3] >= 0, "%s: output %lld: negative extent", who, (long long)i);
        CYB_REQUIRE(o.axis == 1 || o.axis == 2, "%s: output %lld: axis %d is neither 1 nor 2", who, (long long)i, (int)o.axis);
        CYB_REQUIRE_TERM_RANGE(who, i, o, n_terms);
        int64_t total = 1;
        bool fits = true;
        for (int l = 0; l < 4; ++l) {
            fits = fits && o.ext[l] <= kMaxExtent && (o.ext[l] == 0 || total <= (INT64_MAX >> 4) / o.ext[l]);
            total = fits ? total * o.ext[l] : 0;
        }
        CYB_REQUIRE(fits, "%s: output %lld: extent too large", who, (long long)i);
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t)
            CYB_REQUIRE(ht[(size_t)t].K >= 0 && ht[(size_t)t].K <= kMaxExtent, "%s: term %lld: contracted extent %lld is negative or too large", who,
                        (long long)t, (long long)ht[(size_t)t].K);
        if (total == 0) continue;
        CYB_REQUIRE(o.ext[3] == 1 || o.sd[3] == 1, "%s: output %lld: the last level needs the destination stride 1, not %lld", who, (long long)i,
                    (long long)o.sd[3]);
        CYB_REQUIRE(o.dst, "%s: output %lld: dst is NULL", who, (long long)i);
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t)
            CYB_REQUIRE(ht[(size_t)t].K == 0 || (ht[(size_t)t].a && ht[(size_t)t].b), "%s: term %lld: %s is NULL", who, (long long)t,
                        ht[(size_t)t].a ? "b" : "a");
        // pairs of doubles along the fastest level that moves (see the pairing rule above)
        int p = -1;
        for (int l = 0; l < 4; ++l)
            if (o.ext[l] > 1) p = l;
        bool x2 = !CPLX && p >= 0 && o.sd[p] == 1 && even_(o.ext[p]) && ((uintptr_t)o.dst & 15) == 0;
        for (int l = 0; l < p; ++l) x2 = x2 && (o.ext[l] == 1 || even_(o.sd[l]));
        Rec r;
        memset(&r, 0, sizeof(r));
        r.dst = o.dst, r.first_term = o.first_term, r.n_terms = o.n_terms;
        r.mode = CPLX ? kC128 : (x2 ? kF64x2 : kF64);
        r.axis = o.axis, r.pair = x2 ? p : -1;
        // n in registers unless it is the level the flat order walks fastest
        r.n_reg = p != o.axis ? (int32_t)o.ext[o.axis] : 0;
        r.sn = o.sd[o.axis];
        for (int l = 0; l < 4; ++l) {
            r.lv.ext[l] = (int32_t)(l == r.pair ? o.ext[l] / 2 : (r.n_reg && l == o.axis ? 1 : o.ext[l]));
            r.lv.st[0][l] = l == r.pair ? 2 : o.sd[l];
        }
        if (r.n_reg) total /= o.ext[o.axis];
        set_steps(r.lv, 0);
        recs.push_back(r);
        totals.push_back(x2 ? total / 2 : total);
    }
    std::vector<Item> items;
    cut_items(items, recs, totals);
    return launch_items(ctx, compose_weighted_kernel<CPLX>, recs, ht, items, who);
}

} // namespace

extern "C" {

int cyb_compose_weighted_f64(cyb_ctx_t ctx, const cyb_compose_weighted_out* outs, int64_t n_outs, const cyb_compose_weighted_term* terms,
                             int64_t n_terms)
{
    return compose_weighted<false>(ctx, outs, n_outs, terms, n_terms, "cyb_compose_weighted_f64");
}

int cyb_compose_weighted_c128(cyb_ctx_t ctx, const cyb_compose_weighted_out* outs, int64_t n_outs, const cyb_compose_weighted_term* terms,
                              int64_t n_terms)
{
    return compose_weighted<true>(ctx, outs, n_outs, terms, n_terms, "cyb_compose_weighted_c128");
}

} // extern "C"
