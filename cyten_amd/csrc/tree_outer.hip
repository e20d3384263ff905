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
//   * host: the tile is the 4-level index space (ra, rb, ca, cb) in the flat order of dst (cb counts pairs in pair mode).
//     Every record is cut into work items of kMinChunk..kMaxChunk flat units; ONE WAVE owns an item (four items per
//     workgroup, no LDS, no barrier), so that one launch balances thousands of 1 x 1 tiles -- a wave each -- beside a tile of
//     tens of MB.  An item carries the digits and the destination offset of its first unit.
//   * device: a lane keeps a cursor (four digits, destination offset).  It decodes its lane offset (below 64: 32-bit
//     divisions) once per item and then advances by the wave's step of 64 units with the precomputed digits of the step
//     and a precomputed offset correction per wrap of a level: additions and compares only, no division per element.  The
//     source offsets are four multiply-adds per term from the digits.
//   * item, record and term are wave-uniform: their fields travel through scalar loads, the term loop is innermost.
#include "common.h"

#include <algorithm>

namespace {

#define GLOBAL_AS __attribute__((address_space(1)))

constexpr int NT = 256, WAVE = 64, ITEMS_PER_GROUP = NT / WAVE;
constexpr int64_t kMinChunk = 1024, kMaxChunk = 16384, kTargetItems = 8192; // flat units per work item (multiples of WAVE)
typedef double d2 __attribute__((ext_vector_type(2)));
typedef cyb_outer_weighted_out Out;
typedef cyb_outer_weighted_term Term;

// what a lane holds per step: one double, two adjacent doubles, or one complex number
enum { kF64 = 0, kF64x2 = 1, kC128 = 2 };

// one output as the kernel reads it; levels 0..3 = (ra, rb, ca, cb)
struct Rec {
    double* dst;
    int64_t first_term, n_terms;
    int32_t ext[4];
    int32_t step[4]; // digits of the step of WAVE units
    int64_t sd[4];   // destination stride of every level (doubles; kC128: complex elements)
    int64_t wd[4];   // correction of the destination offset when level l wraps: sd[l - 1] - ext[l] * sd[l]
    int64_t step_d;  // increment of the destination offset per step, before corrections
    int32_t mode, reserved;
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

// acc += (c * A) * B of one term at the digits of `c`
template <int MODE> __device__ inline void add_term(typename Acc<MODE>::type& acc, const Term& tm, const Cursor& c)
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
        const d2 x = tm.a_real ? d2{a[oa], 0.0} : *(const GLOBAL_AS d2*)(a + 2 * oa);
        const d2 y = tm.b_real ? d2{b[ob], 0.0} : *(const GLOBAL_AS d2*)(b + 2 * ob);
        const d2 p = d2{tm.coeff_re * x.x - tm.coeff_im * x.y, tm.coeff_re * x.y + tm.coeff_im * x.x};
        acc.x += p.x * y.x - p.y * y.y;
        acc.y += p.x * y.y + p.y * y.x;
    }
}

template <int MODE> __device__ inline void run_item(const Rec& r, const Item& it, const Term* __restrict__ terms, int lane)
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
    for (int64_t k = lane; k < it.count; k += WAVE) {
        T acc;
        if constexpr (MODE == kF64) acc = 0.0; else acc = d2{0.0, 0.0};
        for (int64_t t = r.first_term; t < r.first_term + r.n_terms; ++t) add_term<MODE>(acc, terms[t], c);
        if constexpr (MODE == kF64)
            dst[c.od] = acc;
        else if constexpr (MODE == kF64x2)
            *(GLOBAL_AS d2*)(dst + c.od) = acc;
        else
            *(GLOBAL_AS d2*)(dst + 2 * c.od) = acc;
        advance(c, r, r.step, r.step_d);
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) outer_weighted_kernel(const Rec* __restrict__ recs, const Term* __restrict__ terms,
                                                            const Item* __restrict__ items, int n_items)
{
    // one wave per item: the index is wave-uniform, and so is everything read through it
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ITEMS_PER_GROUP + threadIdx.x / WAVE));
    if (i >= n_items) return;
    const Item& it = items[i];
    const Rec& r = recs[it.rec];
    const int lane = threadIdx.x & (WAVE - 1);
    if constexpr (CPLX) {
        run_item<kC128>(r, it, terms, lane);
    } else {
        if (r.mode == kF64x2)
            run_item<kF64x2>(r, it, terms, lane);
        else
            run_item<kF64>(r, it, terms, lane);
    }
}

inline bool even_(int64_t v) { return (v & 1) == 0; }

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
    int64_t grand = 0;
    for (int64_t i = 0; i < n_outs; ++i) {
        const Out& o = outs[i];
        CYB_REQUIRE(o.ha >= 0 && o.hb >= 0 && o.wa >= 0 && o.wb >= 0, "%s: output %lld: negative extent", who, (long long)i);
        CYB_REQUIRE(o.first_term >= 0 && o.n_terms >= 0 && o.first_term <= n_terms && o.n_terms <= n_terms - o.first_term,
                    "%s: output %lld: bad term range [%lld, +%lld)", who, (long long)i, (long long)o.first_term, (long long)o.n_terms);
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
        r.ext[0] = (int32_t)o.ha, r.ext[1] = (int32_t)o.hb, r.ext[2] = (int32_t)o.wa, r.ext[3] = (int32_t)(o.wb / V);
        r.sd[0] = o.hb * o.ldd, r.sd[1] = o.ldd, r.sd[2] = o.wb, r.sd[3] = V;
        int64_t s = WAVE;
        for (int l = 3; l >= 0; --l) {
            r.wd[l] = (l > 0 ? r.sd[l - 1] : 0) - r.ext[l] * r.sd[l];
            // digits of the step; what is left at the outermost level stays there (a cursor is only read while inside the tile)
            r.step[l] = (int32_t)(l > 0 ? s % r.ext[l] : std::min<int64_t>(s, r.ext[0]));
            s = l > 0 ? s / r.ext[l] : 0;
            r.step_d += r.step[l] * r.sd[l];
        }
        recs.push_back(r);
        totals.push_back(total / V);
        grand += total / V;
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
    hipLaunchKernelGGL(outer_weighted_kernel<CPLX>, dim3(grid), dim3(NT), 0, ctx->stream, static_cast<const Rec*>(d_recs),
                       static_cast<const Term*>(d_terms), static_cast<const Item*>(d_items), (int)items.size());
    CYB_HIP(hipGetLastError());
    return CYB_OK;
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
