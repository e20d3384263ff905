// Grouped tensor product of blocks: every result block of a tensor-level outer in ONE launch.
//
// AbelianBackend::outer (src/backends/abelian.cpp:2794-2850) calls block_backend->tensor_outer once per pair of blocks
// (block_backend.cpp:994-1010: outer, then permute_axes -- a non-contiguous view that the next kernel must copy).  Here a
// record is one pair: dst[i_0..i_{k-1}, j.., i_k..] = a[i..] * b[j..], written C-contiguous in its final axis order, the
// operands read in place through their strides.
//
// The operation is a store stream: one product per output element, sources tiny next to the result.  So the lanes run
// along the flat (contiguous) index of dst and every lane stores 16 bytes per step (two doubles / one complex).
//   * host: the axes of a record in dst order -- head axes of a, axes of b, tail axes of a -- become LEVELS (extent, stride in
//     a, stride in b; one of the two strides is 0).  Extent-1 levels go, adjacent levels whose strides continue each other
//     merge: two contiguous operands give at most 3 levels whatever their rank.
//   * host: every record is cut into work items of at most kMaxChunk flat elements (one workgroup each), so that one launch
//     balances 1-element blocks beside blocks of tens of MB.  An item carries the level digits and the source offsets of its
//     first element.
//   * device: a lane keeps a cursor (digit per level, offset in a, offset in b).  It decodes its start once per item (32-bit
//     divisions of a lane offset below 1024) and then advances by the launch-wide step NT * V with precomputed digits of the
//     step and precomputed offset corrections per wrap of a level: additions and compares only, no division in the loop.
//   * float64: a lane owns the 16-byte aligned pairs of its item (two cursors, one per element of the pair); the one element
//     before the first aligned pair and the one after the last are stored once per item by a single lane.
#include "flat_items.h"

#include <algorithm>

namespace {

constexpr int NT = 256;
constexpr int ML = CYB_MAX_NDIM;
constexpr int64_t kMinChunk = 2048, kMaxChunk = 65536; // flat elements per work item (multiples of 2 * NT)

// one record as the kernel reads it: levels right-aligned (level ML - 1 is the innermost of dst), unused outer levels have
// extent 1 and zeros elsewhere
struct Rec {
    void* dst;
    const void* a;
    const void* b;
    int32_t a_real, b_real;
    int64_t step_a, step_b; // offset increments of one step (sum of step[l] * stride[l])
    int64_t ext[ML];
    int64_t sa[ML], sb[ML];
    int64_t wa[ML], wb[ML]; // offset correction when level l wraps: stride[l - 1] - ext[l] * stride[l]
    int64_t step[ML];       // digits of the step NT * V
};

struct Item {
    int32_t rec;
    int32_t reserved;
    int64_t e0, count; // flat range of dst
    int64_t oa, ob;    // source offsets of element e0
    int64_t idx[ML];   // level digits of element e0
};

template <int L> struct Cursor {
    int64_t idx[L];
    int64_t oa, ob;
};

// c += (digits dg, whose offsets are da / db); every digit below its extent, so a level wraps at most once
template <int L, class D> __device__ inline void advance(Cursor<L>& c, const Rec& r, const D (&dg)[L], int64_t da, int64_t db)
{
    c.oa += da;
    c.ob += db;
    int64_t carry = 0;
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
        const int g = ML - L + l;
        const int64_t i = c.idx[l] + (int64_t)dg[l] + carry;
        const bool w = i >= r.ext[g];
        c.idx[l] = w ? i - r.ext[g] : i;
        c.oa += w ? r.wa[g] : 0;
        c.ob += w ? r.wb[g] : 0;
        carry = w ? 1 : 0;
    }
}

template <class T> struct Elem;
template <> struct Elem<double> {
    static constexpr int V = 2;
    __device__ static inline double value(const Rec& r, int64_t oa, int64_t ob)
    {
        return ((const GLOBAL_AS double*)r.a)[oa] * ((const GLOBAL_AS double*)r.b)[ob];
    }
};
template <> struct Elem<d2> {
    static constexpr int V = 1;
    __device__ static inline d2 load(const void* p, int real, int64_t o)
    {
        if (real) return d2{((const GLOBAL_AS double*)p)[o], 0.0};
        return ((const GLOBAL_AS d2*)p)[o];
    }
    __device__ static inline d2 value(const Rec& r, int64_t oa, int64_t ob)
    {
        const d2 x = load(r.a, r.a_real, oa), y = load(r.b, r.b_real, ob);
        return d2{x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x};
    }
};

template <class T, int L>
__global__ void __launch_bounds__(NT) outer_grouped_kernel(const Rec* __restrict__ recs, const Item* __restrict__ items)
{
    constexpr int V = Elem<T>::V;
    const Item& it = items[blockIdx.x];
    const Rec& r = recs[it.rec];
    const int64_t e0 = it.e0, count = it.count;
    // float64: `head` = 1 if element e0 is not 16-byte aligned; the aligned pairs start behind it
    const int64_t head = V == 2 ? (int64_t)((((uintptr_t)r.dst >> 3) + (uint64_t)e0) & 1) : 0;
    const int64_t n_vec = (count - head) / V; // 16-byte stores of this item
    const bool tail = V == 2 && ((count - head) & 1);

    Cursor<L> c;
    int64_t step[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        c.idx[l] = it.idx[ML - L + l];
        step[l] = r.step[ML - L + l];
    }
    c.oa = it.oa;
    c.ob = it.ob;
    if (V == 2 && head && threadIdx.x == 0) ((GLOBAL_AS double*)r.dst)[e0] = Elem<double>::value(r, c.oa, c.ob);
    {
        // lane offset into the item -> digits (below 1024: 32-bit divisions, extents above it never divide)
        uint32_t d = (uint32_t)head + (uint32_t)threadIdx.x * V;
        uint32_t dg[L];
        int64_t da = 0, db = 0;
#pragma unroll
        for (int l = L - 1; l >= 0; --l) {
            const int g = ML - L + l;
            const uint32_t e32 = r.ext[g] > 1024 ? 1025u : (uint32_t)r.ext[g];
            const uint32_t q = d / e32;
            dg[l] = d - q * e32;
            d = q;
            da += (int64_t)dg[l] * r.sa[g];
            db += (int64_t)dg[l] * r.sb[g];
        }
        advance<L>(c, r, dg, da, db);
    }
    if (V == 2) {
        Cursor<L> c1 = c; // second element of the pair
        int unit[L];
#pragma unroll
        for (int l = 0; l < L; ++l) unit[l] = l == L - 1 ? 1 : 0;
        advance<L>(c1, r, unit, r.sa[ML - 1], r.sb[ML - 1]);
        GLOBAL_AS d2* dst = (GLOBAL_AS d2*)((GLOBAL_AS double*)r.dst + e0 + head);
        int64_t k = threadIdx.x;
        for (; k < n_vec; k += NT) {
            const double v0 = Elem<double>::value(r, c.oa, c.ob);
            const double v1 = Elem<double>::value(r, c1.oa, c1.ob);
            dst[k] = d2{v0, v1};
            advance<L>(c, r, step, r.step_a, r.step_b);
            advance<L>(c1, r, step, r.step_a, r.step_b);
        }
        // the lane whose next pair would start at the last element stores it alone
        if (tail && k == n_vec) ((GLOBAL_AS double*)r.dst)[e0 + count - 1] = Elem<double>::value(r, c.oa, c.ob);
    } else {
        GLOBAL_AS T* dst = (GLOBAL_AS T*)r.dst + e0;
        for (int64_t k = threadIdx.x; k < n_vec; k += NT) {
            dst[k] = Elem<T>::value(r, c.oa, c.ob);
            advance<L>(c, r, step, r.step_a, r.step_b);
        }
    }
}

struct Level {
    int64_t ext, sa, sb;
};

template <class T> int outer_grouped(cyb_ctx_t ctx, const cyb_outer_rec* recs, int64_t n, const char* who)
{
    constexpr int V = Elem<T>::V;
    constexpr bool cplx = V == 1;
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n >= 0 && (n == 0 || recs), "%s: bad list", who);
    std::vector<Rec> dev;
    std::vector<int64_t> totals;
    int max_levels = 0;
    int64_t grand = 0;
    for (int64_t i = 0; i < n; ++i) {
        const cyb_outer_rec& in = recs[i];
        CYB_REQUIRE(in.n_a >= 0 && in.n_b >= 0 && in.n_a + in.n_b <= CYB_MAX_NDIM, "%s: record %lld: %d + %d axes (at most %d)", who,
                    (long long)i, in.n_a, in.n_b, CYB_MAX_NDIM);
        CYB_REQUIRE(in.k >= 0 && in.k <= in.n_a, "%s: record %lld: k = %d outside [0, %d]", who, (long long)i, in.k, in.n_a);
        Level lv[ML];
        int nl = 0;
        int64_t total = 1;
        auto push = [&](int64_t ext, int64_t sa, int64_t sb) {
            total *= ext;
            if (ext == 1) return;
            if (nl > 0 && lv[nl - 1].sa == ext * sa && lv[nl - 1].sb == ext * sb) {
                lv[nl - 1] = Level{lv[nl - 1].ext * ext, sa, sb}; // the outer level continues into this one
                return;
            }
            lv[nl++] = Level{ext, sa, sb};
        };
        bool neg = false;
        for (int k = 0; k < in.n_a; ++k) neg = neg || in.a_shape[k] < 0;
        for (int k = 0; k < in.n_b; ++k) neg = neg || in.b_shape[k] < 0;
        CYB_REQUIRE(!neg, "%s: record %lld: negative extent", who, (long long)i);
        for (int k = 0; k < in.k; ++k) push(in.a_shape[k], in.a_strides[k], 0);
        for (int k = 0; k < in.n_b; ++k) push(in.b_shape[k], 0, in.b_strides[k]);
        for (int k = in.k; k < in.n_a; ++k) push(in.a_shape[k], in.a_strides[k], 0);
        if (total == 0) continue;
        CYB_REQUIRE(in.dst && in.a && in.b, "%s: record %lld: %s is NULL", who, (long long)i, !in.dst ? "dst" : (!in.a ? "a" : "b"));
        const bool a_real = !cplx || in.a_is_real, b_real = !cplx || in.b_is_real;
        CYB_REQUIRE((uintptr_t)in.dst % (cplx ? 16 : 8) == 0 && (uintptr_t)in.a % (a_real ? 8 : 16) == 0 &&
                        (uintptr_t)in.b % (b_real ? 8 : 16) == 0,
                    "%s: record %lld: misaligned pointer", who, (long long)i);
        Rec r;
        memset(&r, 0, sizeof(r));
        r.dst = in.dst, r.a = in.a, r.b = in.b;
        r.a_real = a_real, r.b_real = b_real;
        for (int g = 0; g < ML; ++g) r.ext[g] = 1;
        int64_t s = (int64_t)NT * V;
        for (int l = nl - 1; l >= 0; --l) {
            const int g = ML - nl + l;
            r.ext[g] = lv[l].ext, r.sa[g] = lv[l].sa, r.sb[g] = lv[l].sb;
            r.wa[g] = (l > 0 ? lv[l - 1].sa : 0) - lv[l].ext * lv[l].sa;
            r.wb[g] = (l > 0 ? lv[l - 1].sb : 0) - lv[l].ext * lv[l].sb;
            // digits of the step; what is left at the outermost level stays there (a cursor is only read while inside the record)
            r.step[g] = l > 0 ? s % lv[l].ext : s;
            s = l > 0 ? s / lv[l].ext : 0;
            r.step_a += r.step[g] * r.sa[g];
            r.step_b += r.step[g] * r.sb[g];
        }
        dev.push_back(r);
        totals.push_back(total);
        max_levels = std::max(max_levels, nl);
        grand += total;
    }
    if (dev.empty()) return CYB_OK;
    // about 4096 workgroups for a large launch; an item is a multiple of 2 * NT elements so that every item of a record
    // sees the same 16-byte alignment
    int64_t chunk = (grand / 4096 + 2 * NT - 1) / (2 * NT) * (2 * NT);
    chunk = std::min(std::max(chunk, kMinChunk), kMaxChunk);
    std::vector<Item> items;
    for (size_t i = 0; i < dev.size(); ++i) {
        const Rec& r = dev[i];
        for (int64_t e0 = 0; e0 < totals[i]; e0 += chunk) {
            Item it;
            memset(&it, 0, sizeof(it));
            it.rec = (int32_t)i;
            it.e0 = e0, it.count = std::min(chunk, totals[i] - e0);
            int64_t e = e0;
            for (int g = ML - 1; g >= 0; --g) {
                it.idx[g] = e % r.ext[g];
                e /= r.ext[g];
                it.oa += it.idx[g] * r.sa[g];
                it.ob += it.idx[g] * r.sb[g];
            }
            items.push_back(it);
        }
    }
    return cyb_flat::launch(ctx, who, max_levels <= 3 ? outer_grouped_kernel<T, 3> : outer_grouped_kernel<T, ML>, cyb_flat::arrays(dev, items));
}

} // namespace

extern "C" {

int cyb_outer_grouped_f64(cyb_ctx_t ctx, const cyb_outer_rec* recs, int64_t n)
{
    return outer_grouped<double>(ctx, recs, n, "cyb_outer_grouped_f64");
}

int cyb_outer_grouped_c128(cyb_ctx_t ctx, const cyb_outer_rec* recs, int64_t n)
{
    return outer_grouped<d2>(ctx, recs, n, "cyb_outer_grouped_c128");
}

} // extern "C"
