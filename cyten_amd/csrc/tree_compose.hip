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
//   * host: every record is cut into work items of kMinChunk..kMaxChunk flat units; ONE WAVE owns an item (four items per
//     workgroup, no LDS, no barrier), so that one launch balances thousands of 1 x 1 tiles -- a wave each -- beside a tile of
//     tens of MB.  An item carries the digits and the destination offset of its first unit.
//   * device: a lane keeps a cursor (four digits, destination offset), decodes its lane offset once per item (below 64:
//     32-bit divisions) and then advances by the wave's step of 64 units with precomputed digits and a precomputed offset
//     correction per wrap of a level: additions and compares only, no division per element.  The source offsets are four
//     multiply-adds per term from the digits.
//   * item, record and term are wave-uniform: their fields travel through scalar loads; the k loop is innermost.
#include "common.h"

#include <algorithm>

namespace {

#define GLOBAL_AS __attribute__((address_space(1)))

constexpr int NT = 256, WAVE = 64, ITEMS_PER_GROUP = NT / WAVE;
constexpr int64_t kMinChunk = 1024, kMaxChunk = 16384, kTargetItems = 8192; // flat units per work item (multiples of WAVE)
constexpr int64_t kMaxExtent = (int64_t)1 << 30;
constexpr int kNB = 4; // values of n a lane holds in registers at a time
typedef double d2 __attribute__((ext_vector_type(2)));
typedef cyb_compose_weighted_out Out;
typedef cyb_compose_weighted_term Term;

// what a lane holds per step: one double, two adjacent doubles, or one complex number
enum { kF64 = 0, kF64x2 = 1, kC128 = 2 };

// one output as the kernel reads it
struct Rec {
    double* dst;
    int64_t first_term, n_terms;
    int32_t ext[4];  // (kF64x2: ext[pair] counts pairs)
    int32_t step[4]; // digits of the step of WAVE units
    int64_t sd[4];   // destination stride of every level (doubles; kC128: complex elements)
    int64_t wd[4];   // correction of the destination offset when level l wraps: sd[l - 1] - ext[l] * sd[l]
    int64_t step_d;  // increment of the destination offset per step, before corrections
    int32_t mode, axis, pair;           // pair: the level that counts pairs (kF64x2), else -1
    int32_t n_reg;                      // n in registers: its extent N (ext[axis] is 1 then); 0: n runs in the lanes
    int64_t sn;                         // destination stride of n (as sd)
};

struct Item {
    int32_t rec;
    int32_t reserved;
    int64_t count;  // flat units of this item
    int64_t od;     // destination offset of its first unit (doubles; kC128: complex elements)
    int32_t idx[4]; // digits of its first unit
};

struct Cursor {
    int32_t idx[4];
    int64_t od;
};

// c += (digits dg, whose destination offset is dd); every digit below its extent, so a level wraps at most once
__device__ inline void advance(Cursor& c, const Rec& r, const int32_t (&dg)[4], int64_t dd)
{
    c.od += dd;
    int32_t carry = 0;
#pragma unroll
    for (int l = 3; l >= 0; --l) {
        const int32_t i = c.idx[l] + dg[l] + carry;
        const bool w = i >= r.ext[l];
        c.idx[l] = w ? i - r.ext[l] : i;
        c.od += w ? r.wd[l] : 0;
        carry = w ? 1 : 0;
    }
}

template <int MODE> struct Acc { typedef d2 type; };
template <> struct Acc<kF64> { typedef double type; };

// acc += c * sum_k A[k] * B[k] of one term at the digits of `c`
template <int MODE> __device__ inline void add_term(typename Acc<MODE>::type& acc, const Term& tm, const Rec& r, const Cursor& c)
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
            const d2 x = tm.a_real ? d2{a[ia], 0.0} : *(const GLOBAL_AS d2*)(a + 2 * ia);
            const d2 y = tm.b_real ? d2{b[ib], 0.0} : *(const GLOBAL_AS d2*)(b + 2 * ib);
            s.x += x.x * y.x - x.y * y.y;
            s.y += x.x * y.y + x.y * y.x;
        }
        acc.x += tm.coeff_re * s.x - tm.coeff_im * s.y;
        acc.y += tm.coeff_re * s.y + tm.coeff_im * s.x;
    }
}

// acc[j] += c * sum_k A[k] * B_{n0 + j}[k], j < nn <= kNB, of one term at the digits of `c` (whose digit of `axis` is 0)
template <int MODE>
__device__ inline void add_term_block(typename Acc<MODE>::type (&acc)[kNB], const Term& tm, const Rec& r, const Cursor& c, int32_t n0, int32_t nn)
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
            const d2 x = tm.a_real ? d2{a[ia], 0.0} : *(const GLOBAL_AS d2*)(a + 2 * ia);
#pragma unroll
            for (int j = 0; j < kNB; ++j)
                if (j < nn) {
                    const int64_t ib = ob + j * tm.b_ns + k * kb;
                    const d2 y = tm.b_real ? d2{b[ib], 0.0} : *(const GLOBAL_AS d2*)(b + 2 * ib);
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
    typedef typename Acc<MODE>::type T;
    Cursor c;
#pragma unroll
    for (int l = 0; l < 4; ++l) c.idx[l] = it.idx[l];
    c.od = it.od;
    {
        // lane offset into the item -> digits (below 64: 32-bit divisions, extents above it never divide)
        uint32_t d = (uint32_t)lane;
        int32_t dg[4];
#pragma unroll
        for (int l = 3; l >= 0; --l) {
            const uint32_t e32 = r.ext[l] > WAVE ? (uint32_t)WAVE + 1 : (uint32_t)r.ext[l];
            const uint32_t q = d / e32;
            dg[l] = (int32_t)(d - q * e32);
            d = q;
        }
        advance(c, r, dg, dg[0] * r.sd[0] + dg[1] * r.sd[1] + dg[2] * r.sd[2] + dg[3] * r.sd[3]);
    }
    GLOBAL_AS double* dst = (GLOBAL_AS double*)r.dst;
    for (int64_t u = lane; u < it.count; u += WAVE) {
        if constexpr (NREG) {
            for (int32_t n0 = 0; n0 < r.n_reg; n0 += kNB) {
                const int32_t nn = r.n_reg - n0 < kNB ? r.n_reg - n0 : kNB;
                T acc[kNB] = {};
                for (int64_t t = r.first_term; t < r.first_term + r.n_terms; ++t) add_term_block<MODE>(acc, terms[t], r, c, n0, nn);
#pragma unroll
                for (int j = 0; j < kNB; ++j)
                    if (j < nn) {
                        const int64_t od = c.od + (int64_t)(n0 + j) * r.sn;
                        if constexpr (MODE == kF64)
                            dst[od] = acc[j];
                        else if constexpr (MODE == kF64x2)
                            *(GLOBAL_AS d2*)(dst + od) = acc[j];
                        else
                            *(GLOBAL_AS d2*)(dst + 2 * od) = acc[j];
                    }
            }
        } else {
            T acc;
            if constexpr (MODE == kF64) acc = 0.0; else acc = d2{0.0, 0.0};
            for (int64_t t = r.first_term; t < r.first_term + r.n_terms; ++t) add_term<MODE>(acc, terms[t], r, c);
            if constexpr (MODE == kF64)
                dst[c.od] = acc;
            else if constexpr (MODE == kF64x2)
                *(GLOBAL_AS d2*)(dst + c.od) = acc;
            else
                *(GLOBAL_AS d2*)(dst + 2 * c.od) = acc;
        }
        advance(c, r, r.step, r.step_d);
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) compose_weighted_kernel(const Rec* __restrict__ recs, const Term* __restrict__ terms,
                                                              const Item* __restrict__ items, int n_items)
{
    // one wave per item: the index is wave-uniform, and so is everything read through it
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ITEMS_PER_GROUP + threadIdx.x / WAVE));
    if (i >= n_items) return;
    const Item& it = items[i];
    const Rec& r = recs[it.rec];
    const int lane = threadIdx.x & (WAVE - 1);
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

inline bool even_(int64_t v) { return (v & 1) == 0; }

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
    int64_t grand = 0;
    for (int64_t i = 0; i < n_outs; ++i) {
        const Out& o = outs[i];
        CYB_REQUIRE(o.ext[0] >= 0 && o.ext[1] >= 0 && o.ext[2] >= 0 && o.ext[3] >= 0, "%s: output %lld: negative extent", who, (long long)i);
        CYB_REQUIRE(o.axis == 1 || o.axis == 2, "%s: output %lld: axis %d is neither 1 nor 2", who, (long long)i, (int)o.axis);
        CYB_REQUIRE(o.first_term >= 0 && o.n_terms >= 0 && o.first_term <= n_terms && o.n_terms <= n_terms - o.first_term,
                    "%s: output %lld: bad term range [%lld, +%lld)", who, (long long)i, (long long)o.first_term, (long long)o.n_terms);
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
            r.ext[l] = (int32_t)(l == r.pair ? o.ext[l] / 2 : (r.n_reg && l == o.axis ? 1 : o.ext[l]));
            r.sd[l] = l == r.pair ? 2 : o.sd[l];
        }
        if (r.n_reg) total /= o.ext[o.axis];
        int64_t s = WAVE;
        for (int l = 3; l >= 0; --l) {
            r.wd[l] = (l > 0 ? r.sd[l - 1] : 0) - r.ext[l] * r.sd[l];
            // digits of the step; what is left at the outermost level stays there (a cursor is only read while inside the tile)
            r.step[l] = (int32_t)(l > 0 ? s % r.ext[l] : std::min<int64_t>(s, r.ext[0]));
            s = l > 0 ? s / r.ext[l] : 0;
            r.step_d += r.step[l] * r.sd[l];
        }
        recs.push_back(r);
        totals.push_back(x2 ? total / 2 : total);
        grand += totals.back();
    }
    if (recs.empty()) return CYB_OK;
    // about kTargetItems waves for a large launch
    int64_t chunk = (grand / kTargetItems + WAVE - 1) / WAVE * WAVE;
    chunk = std::min(std::max(chunk, kMinChunk), kMaxChunk);
    std::vector<Item> items;
    for (size_t i = 0; i < recs.size(); ++i) {
        const Rec& r = recs[i];
        for (int64_t e0 = 0; e0 < totals[i]; e0 += chunk) {
            Item it;
            memset(&it, 0, sizeof(it));
            it.rec = (int32_t)i;
            it.count = std::min(chunk, totals[i] - e0);
            int64_t e = e0;
            for (int l = 3; l >= 0; --l) {
                it.idx[l] = (int32_t)(e % r.ext[l]);
                e /= r.ext[l];
                it.od += it.idx[l] * r.sd[l];
            }
            items.push_back(it);
        }
    }
    CYB_REQUIRE(items.size() < ((size_t)1 << 31), "%s: too many work items", who);
    void *d_recs = nullptr, *d_terms = nullptr, *d_items = nullptr;
    CYB_TRY(cyb::upload_packed(ctx, {{recs.data(), sizeof(Rec) * recs.size(), &d_recs},
                                     {ht.empty() ? (const void*)recs.data() : (const void*)ht.data(), ht.empty() ? 8 : sizeof(Term) * ht.size(), &d_terms},
                                     {items.data(), sizeof(Item) * items.size(), &d_items}}));
    const unsigned grid = (unsigned)((items.size() + ITEMS_PER_GROUP - 1) / ITEMS_PER_GROUP);
    hipLaunchKernelGGL(compose_weighted_kernel<CPLX>, dim3(grid), dim3(NT), 0, ctx->stream, static_cast<const Rec*>(d_recs),
                       static_cast<const Term*>(d_terms), static_cast<const Item*>(d_items), (int)items.size());
    CYB_HIP(hipGetLastError());
    return CYB_OK;
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
