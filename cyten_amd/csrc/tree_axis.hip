// Axis operations on the tree blocks of fusion-tree tensors, and the quantum-dimension weighted reduction (gfx950).
//
// FusionTreeBackend::scale_axis (src/backends/fusion_tree_backend.cpp:3521-3644) and ::_mask_contract (:2372-2500) work
// per forest block: slice the coupled block, reshape to the multiplicities, scale_axis / apply_mask / enlarge_leg, reshape
// back, set_item -- five block-backend calls per forest, hundreds to thousands of them per SU(2) tensor.  Here a record is one
// tree block of one coupled block: the rows (codomain) or columns (domain) [start, start + outer * A * inner) of the block,
// read in place through the block's own strides and written in place into the rows / columns [start', ...) of the result
// block.  One launch covers all records of a tensor operation.
//
//   tree position t = (o * A + a) * inner + i,  other matrix index x in [0, X)
//   scale   : dst[t, x] = f[a] * src[t, x]                              (A' = A)
//   gather  : dst[(o * A' + a') * inner + i, x] = src[(o * A + idx[a']) * inner + i, x]     (apply_mask)
//   scatter : dst[(o * A' + idx[a]) * inner + i, x] = src[(o * A + a) * inner + i, x]        (enlarge_leg; the entry
//             point zero-fills the regions the caller lists before the launch)
//
// Memory-bound work, organised like blockops.hip: records are cut into work items of chunk_real(total) elements (flat_items.h), one
// workgroup each.  Lanes run along whichever matrix index has unit stride in the destination.  Where that index has unit
// stride in the source too and the contiguous run is at least 16 elements long a wave owns a run: the run's offsets (and
// its factor, if it has one) are decoded once; the four waves share a run of 2048 elements or more.  Float64 runs whose
// two sides share their 16-byte phase move as 16-byte loads and stores (one element peeled in front if needed), all others
// as 8-byte ones.  Short or strided runs take the
// per-element path (index arithmetic in 32 bits when the record allows).  Complex data is interleaved (re, im): one 16-byte
// access per element; a float64 source under the complex entry is widened on load.
//
// cyb_dot_weighted_*: sum_n w_n <x_n, y_n> over 2-D strided views in two stages of fixed order (no float atomics,
// bit-identical from run to run): FusionTreeBackend::inner (:1238-1259), ::norm (:1280-1296) and, with the diagonal as a
// one-column view against a constant one, ::trace_full (:1261-1278) -- one launch chain instead of a reduction and a host
// wait per coupled sector.
#include "flat_items.h"

#include <algorithm>

namespace {

using namespace cyb_flat; // Item, NT, chunk_real, cut, launch, the fixed-order reduction

enum { LAY_ELEM_X = 0, LAY_ELEM_T, LAY_RUN_X, LAY_RUN_T_SCALE, LAY_RUN_T_INNER };

struct Rec {
    const void* src;
    void* dst;
    const void* table;
    int64_t s_ts, s_xs, d_ts, d_xs; // strides of the tree index / the other index, elements of the operand's own type
    int64_t s0, d0;                 // start of the tree block
    int64_t X, outer, As, Ad, inner;
    int64_t Ai, Ti;                 // iterated extent of the acted leg (gather: A', else A) and of the tree index
    int64_t R;                      // run length of the run layouts
    int32_t mode, src_real, f_complex, layout, small, pad;
};

template <class T> struct Ops;
template <> struct Ops<double> {
    typedef double F;
    __device__ static inline double load(const Rec& r, int64_t o) { return ((gcp)r.src)[o]; }
    __device__ static inline void store(const Rec& r, int64_t o, double v) { ((gp)r.dst)[o] = v; }
    __device__ static inline double factor(const Rec& r, int64_t a) { return ((gcp)r.table)[a]; }
    __device__ static inline double one() { return 1.0; }
    __device__ static inline double mul(double v, double f) { return v * f; }
};
template <> struct Ops<d2> {
    typedef d2 F;
    __device__ static inline d2 load(const Rec& r, int64_t o)
    {
        if (r.src_real) return d2{((gcp)r.src)[o], 0.0};
        return ((const GLOBAL_AS d2*)r.src)[o];
    }
    __device__ static inline void store(const Rec& r, int64_t o, d2 v) { ((GLOBAL_AS d2*)r.dst)[o] = v; }
    __device__ static inline d2 factor(const Rec& r, int64_t a)
    {
        if (r.f_complex) return ((const GLOBAL_AS d2*)r.table)[a];
        return d2{((gcp)r.table)[a], 0.0};
    }
    __device__ static inline d2 one() { return d2{1.0, 0.0}; }
    // two products and one sum per component, none of them fused, so that the result is the one of numpy's arithmetic on
    // separately rounded products.  The library is built with -ffp-contract=fast, which contracts a * b - c * d whatever a
    // pragma says: every product passes through an empty asm statement, behind which the compiler cannot see a multiply.
    __device__ static inline double rounded(double p)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(p));
#endif
        return p;
    }
    __device__ static inline d2 mul(d2 v, d2 f)
    {
        if (f.y == 0.0) return d2{v.x * f.x, v.y * f.x};
        return d2{rounded(v.x * f.x) - rounded(v.y * f.y), rounded(v.x * f.y) + rounded(v.y * f.x)};
    }
};

// iterated tree position t -> (position in the source tree block, position in the destination tree block, index a of the factor)
template <class I> __device__ inline void tree_pos(const Rec& r, I t, int64_t& ts, int64_t& td, int64_t& a)
{
    if (r.mode == CYB_TREE_SCALE) {
        ts = td = (int64_t)t;
        a = (int64_t)((t / (I)r.inner) % (I)r.Ai);
        return;
    }
    const I q = t / (I)r.inner, i = t - q * (I)r.inner;
    const I o = q / (I)r.Ai, ai = q - o * (I)r.Ai;
    const int64_t k = ((const GLOBAL_AS int64_t*)r.table)[ai];
    a = 0;
    if (r.mode == CYB_TREE_GATHER) {
        ts = ((int64_t)o * r.As + k) * r.inner + (int64_t)i;
        td = (int64_t)t;
    } else {
        ts = (int64_t)t;
        td = ((int64_t)o * r.Ad + k) * r.inner + (int64_t)i;
    }
}

template <class T, class I> __device__ inline void elem_path(const Rec& r, const Item& it)
{
    const bool tfast = r.layout == LAY_ELEM_T;
    const I e1 = (I)(it.start + it.count);
    for (I e = (I)it.start + threadIdx.x; e < e1; e += NT) {
        I t, x;
        if (tfast) {
            x = e / (I)r.Ti;
            t = e - x * (I)r.Ti;
        } else {
            t = e / (I)r.X;
            x = e - t * (I)r.X;
        }
        int64_t ts, td, a;
        tree_pos<I>(r, t, ts, td, a);
        const T v = Ops<T>::load(r, (r.s0 + ts) * r.s_ts + (int64_t)x * r.s_xs);
        const int64_t dof = (r.d0 + td) * r.d_ts + (int64_t)x * r.d_xs;
        Ops<T>::store(r, dof, r.mode == CYB_TREE_SCALE ? Ops<T>::mul(v, Ops<T>::factor(r, a)) : v);
    }
}

// factor of position p of a t-fast scale run
struct VarFactor {
    const Rec& r;
    __device__ inline double operator()(int64_t p) const { return ((gcp)r.table)[(p / r.inner) % r.Ai]; }
};
struct ConstFactor {
    double f;
    __device__ inline double operator()(int64_t) const { return f; }
};

// one wave moves elements [c0, c1) of a float64 run: dst[so.. ] = src[..] * fac(position)
// (W = 64: the calling wave owns the run; W = NT: the whole workgroup shares it, lane = threadIdx.x)
template <class Fac> __device__ inline void run_f64(gcp sp, gp dp, int64_t c0, int64_t c1, int lane, int W, const Fac& fac)
{
    sp += c0, dp += c0;
    int64_t n = c1 - c0, p = c0;
    if (n <= 0) return;
    const unsigned ms = (unsigned)((uintptr_t)sp & 15), md = (unsigned)((uintptr_t)dp & 15);
    if (ms != md) { // the two sides never meet a common 16-byte boundary: 8-byte accesses
        for (int64_t i = lane; i < n; i += W) dp[i] = sp[i] * fac(p + i);
        return;
    }
    if (ms) {
        if (lane == 0) dp[0] = sp[0] * fac(p);
        ++sp, ++dp, ++p, --n;
    }
    const GLOBAL_AS d2* sv = (const GLOBAL_AS d2*)sp;
    GLOBAL_AS d2* dv = (GLOBAL_AS d2*)dp;
    const int64_t nv = n >> 1;
    for (int64_t i = lane; i < nv; i += W) {
        const d2 v = sv[i];
        dv[i] = d2{v.x * fac(p + 2 * i), v.y * fac(p + 2 * i + 1)};
    }
    if ((n & 1) && lane == 0) dp[n - 1] = sp[n - 1] * fac(p + n - 1);
}

template <class T> __device__ inline void run_path(const Rec& r, const Item& it)
{
    const int64_t R = r.R;
    const int64_t e0 = it.start, e1 = it.start + it.count;
    const int64_t r0 = e0 / R, r1 = (e1 - 1) / R;
    // short runs: one wave per run (four runs in flight per workgroup); long runs, of which a work item holds one or
    // two: the waves share a run
    const bool shared = R >= 2048;
    const int wave = shared ? 0 : (int)(threadIdx.x >> 6), lane = shared ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    const int W = shared ? NT : 64;
    for (int64_t row = r0 + wave; row <= r1; row += shared ? 1 : NT / 64) {
        const int64_t c0 = (row == r0) ? e0 - r0 * R : 0;
        const int64_t c1 = (row == r1) ? e1 - r1 * R : R;
        int64_t so, dof, a = 0; // offsets of element 0 of the run
        if (r.layout == LAY_RUN_X) { // the run is x in [0, X) of tree position `row`
            int64_t ts, td;
            tree_pos<int64_t>(r, row, ts, td, a);
            so = (r.s0 + ts) * r.s_ts;
            dof = (r.d0 + td) * r.d_ts;
        } else if (r.layout == LAY_RUN_T_SCALE) { // the run is the whole tree block at x = row
            so = r.s0 + row * r.s_xs;
            dof = r.d0 + row * r.d_xs;
        } else { // the run is i in [0, inner) at (x, o, a): row = x * (outer * Ai) + (o * Ai + a)
            const int64_t per_x = r.outer * r.Ai;
            const int64_t x = row / per_x, q = row - x * per_x;
            int64_t ts, td;
            tree_pos<int64_t>(r, q * r.inner, ts, td, a);
            so = r.s0 + ts + x * r.s_xs;
            dof = r.d0 + td + x * r.d_xs;
        }
        if constexpr (sizeof(T) == 8) {
            gcp sp = (gcp)r.src + so;
            gp dp = (gp)r.dst + dof;
            if (r.layout == LAY_RUN_T_SCALE) run_f64(sp, dp, c0, c1, lane, W, VarFactor{r});
            else run_f64(sp, dp, c0, c1, lane, W, ConstFactor{r.mode == CYB_TREE_SCALE ? Ops<double>::factor(r, a) : 1.0});
        } else {
            if (r.mode != CYB_TREE_SCALE) {
                for (int64_t i = c0 + lane; i < c1; i += W) Ops<T>::store(r, dof + i, Ops<T>::load(r, so + i));
            } else if (r.layout == LAY_RUN_T_SCALE) {
                for (int64_t i = c0 + lane; i < c1; i += W)
                    Ops<T>::store(r, dof + i, Ops<T>::mul(Ops<T>::load(r, so + i), Ops<T>::factor(r, (i / r.inner) % r.Ai)));
            } else {
                const T f = Ops<T>::factor(r, a);
                for (int64_t i = c0 + lane; i < c1; i += W) Ops<T>::store(r, dof + i, Ops<T>::mul(Ops<T>::load(r, so + i), f));
            }
        }
    }
}

template <class T> __global__ void __launch_bounds__(NT) tree_axis_kernel(const Rec* __restrict__ recs, const Item* __restrict__ items)
{
    const Item it = items[blockIdx.x];
    const Rec& r = recs[it.desc];
    if (r.layout >= LAY_RUN_X) run_path<T>(r, it);
    else if (r.small) elem_path<T, uint32_t>(r, it);
    else elem_path<T, int64_t>(r, it);
}

template <class T> int tree_axis(cyb_ctx_t ctx, const cyb_tree_axis_rec* recs, int64_t n, const cyb_tree_fill* fills, int64_t n_fills,
                                 const char* who)
{
    constexpr bool cplx = sizeof(T) == 16;
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n >= 0 && (n == 0 || recs), "%s: bad record list", who);
    CYB_REQUIRE(n_fills >= 0 && (n_fills == 0 || fills), "%s: bad fill list", who);
    for (int64_t i = 0; i < n_fills; ++i) {
        CYB_REQUIRE(fills[i].bytes >= 0, "%s: fill %lld: negative size", who, (long long)i);
        CYB_REQUIRE(fills[i].bytes == 0 || fills[i].ptr, "%s: fill %lld: NULL pointer", who, (long long)i);
    }
    std::vector<Rec> dev;
    std::vector<int64_t> totals;
    const int64_t lim = (int64_t)1 << 31;
    for (int64_t i = 0; i < n; ++i) {
        const cyb_tree_axis_rec& in = recs[i];
        CYB_REQUIRE(in.mode == CYB_TREE_SCALE || in.mode == CYB_TREE_GATHER || in.mode == CYB_TREE_SCATTER, "%s: record %lld: unknown mode %d",
                    who, (long long)i, in.mode);
        CYB_REQUIRE(in.X >= 0 && in.outer >= 0 && in.A >= 0 && in.A_dst >= 0 && in.inner >= 0, "%s: record %lld: negative extent", who,
                    (long long)i);
        CYB_REQUIRE(in.src_start >= 0 && in.dst_start >= 0, "%s: record %lld: negative start", who, (long long)i);
        CYB_REQUIRE(in.mode != CYB_TREE_SCALE || in.A_dst == in.A, "%s: record %lld: scale needs A' = A", who, (long long)i);
        CYB_REQUIRE(in.mode != CYB_TREE_GATHER || in.A_dst <= in.A, "%s: record %lld: gather needs A' <= A (%lld > %lld)", who, (long long)i,
                    (long long)in.A_dst, (long long)in.A);
        CYB_REQUIRE(in.mode != CYB_TREE_SCATTER || in.A <= in.A_dst, "%s: record %lld: scatter needs A <= A' (%lld > %lld)", who,
                    (long long)i, (long long)in.A, (long long)in.A_dst);
        const int64_t Ai = in.mode == CYB_TREE_GATHER ? in.A_dst : in.A;
        int64_t Ti = 0, total = 0, big = 0;
        CYB_REQUIRE(!__builtin_mul_overflow(in.outer, std::max(in.A, in.A_dst), &big) && !__builtin_mul_overflow(big, in.inner, &big) &&
                        !__builtin_mul_overflow(big, in.X, &total),
                    "%s: record %lld: extents overflow", who, (long long)i);
        Ti = in.outer * Ai * in.inner, total = Ti * in.X;
        if (total == 0) continue;
        CYB_REQUIRE(in.src && in.dst && in.table, "%s: record %lld: %s is NULL", who, (long long)i,
                    !in.src ? "src" : (!in.dst ? "dst" : "table"));
        const bool src_real = !cplx || in.src_is_real, f_complex = cplx && in.table_is_complex;
        CYB_REQUIRE((uintptr_t)in.dst % (cplx ? 16 : 8) == 0 && (uintptr_t)in.src % (src_real ? 8 : 16) == 0 &&
                        (uintptr_t)in.table % (in.mode == CYB_TREE_SCALE && f_complex ? 16 : 8) == 0,
                    "%s: record %lld: misaligned pointer", who, (long long)i);
        Rec r;
        memset(&r, 0, sizeof(r));
        r.src = in.src, r.dst = in.dst, r.table = in.table;
        r.s_ts = in.src_ts, r.s_xs = in.src_xs, r.d_ts = in.dst_ts, r.d_xs = in.dst_xs;
        r.s0 = in.src_start, r.d0 = in.dst_start;
        r.X = in.X, r.outer = in.outer, r.As = in.A, r.Ad = in.A_dst, r.inner = in.inner;
        r.Ai = Ai, r.Ti = Ti;
        r.mode = in.mode, r.src_real = cplx && src_real, r.f_complex = f_complex;
        r.small = total < lim && in.outer * std::max(in.A, in.A_dst) * in.inner < lim;
        // lanes along the index with unit stride in the destination
        const bool tfast = in.dst_ts == 1 && (in.dst_xs != 1 || in.X <= 1);
        r.layout = tfast ? LAY_ELEM_T : LAY_ELEM_X;
        r.R = 1;
        if (!tfast && in.src_xs == 1 && in.dst_xs == 1 && in.X >= 16) {
            r.layout = LAY_RUN_X, r.R = in.X;
        } else if (tfast && in.src_ts == 1 && in.mode == CYB_TREE_SCALE && Ti >= 16) {
            r.layout = LAY_RUN_T_SCALE, r.R = Ti;
        } else if (tfast && in.src_ts == 1 && in.mode != CYB_TREE_SCALE && in.inner >= 16) {
            r.layout = LAY_RUN_T_INNER, r.R = in.inner;
        }
        dev.push_back(r);
        totals.push_back(total);
    }
    // everything is validated: from here on work is enqueued
    for (int64_t i = 0; i < n_fills; ++i)
        if (fills[i].bytes > 0) CYB_HIP(hipMemsetAsync(fills[i].ptr, 0, (size_t)fills[i].bytes, ctx->stream));
    std::vector<Item> items;
    CYB_CUT(who, items, totals, chunk_real(sum_of(totals)));
    return launch(ctx, who, tree_axis_kernel<T>, arrays(dev, items));
}

// ---------------------------------------------------------------------------------------------
// weighted reduction
struct WDot {
    const double* x;
    const double* y; // NULL: x itself
    int64_t rows, cols, x_rs, x_cs, y_rs, y_cs;
    double w;
    int32_t flat, pad; // both operands contiguous: element e of the flat range is at offset e
};

// partial[C * item + c] = w * sum over the item's elements; complex: (re, im) of conj?(x) y
template <bool CPLX>
__global__ void __launch_bounds__(NT) wdot_stage1_kernel(const WDot* __restrict__ descs, const Item* __restrict__ items,
                                                         double* __restrict__ partial, int conj_x)
{
    constexpr int C = CPLX ? 2 : 1;
    __shared__ double red[C][WAVES];
    const Item it = items[blockIdx.x];
    const WDot d = descs[it.desc];
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    const double sgn = conj_x ? -1.0 : 1.0;
    for (int64_t e = it.start + threadIdx.x; e < it.start + it.count; e += NT) {
        int64_t xo = e, yo = e;
        if (!d.flat) {
            const int64_t rr = e / d.cols, cc = e - rr * d.cols;
            xo = rr * d.x_rs + cc * d.x_cs;
            yo = rr * d.y_rs + cc * d.y_cs;
        }
        if constexpr (CPLX) {
            d2 a = ((const GLOBAL_AS d2*)d.x)[xo];
            const d2 b = d.y ? ((const GLOBAL_AS d2*)d.y)[yo] : a;
            a.y *= sgn;
            acc[0] += a.x * b.x - a.y * b.y;
            acc[1] += a.x * b.y + a.y * b.x;
        } else {
            const double a = ((gcp)d.x)[xo];
            acc[0] += a * (d.y ? ((gcp)d.y)[yo] : a);
        }
    }
    block_reduce<C>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) partial[C * (int64_t)blockIdx.x + c] = d.w * acc[c];
    }
}

template <bool CPLX> int dot_weighted(cyb_ctx_t ctx, const cyb_wdot_desc* descs, int64_t n, int conj_x, double* result_dev, const char* who)
{
    constexpr int C = CPLX ? 2 : 1;
    CYB_REQUIRE(ctx && result_dev, "%s: NULL argument", who);
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "%s: bad descriptor list", who);
    std::vector<WDot> hd;
    std::vector<int64_t> totals;
    for (int64_t i = 0; i < n; ++i) {
        const cyb_wdot_desc& d = descs[i];
        CYB_REQUIRE(d.rows >= 0 && d.cols >= 0, "%s: desc %lld: negative extent", who, (long long)i);
        int64_t total = 0;
        CYB_REQUIRE(!__builtin_mul_overflow(d.rows, d.cols, &total), "%s: desc %lld: extents overflow", who, (long long)i);
        if (total == 0) continue;
        CYB_REQUIRE(d.x, "%s: desc %lld: x is NULL", who, (long long)i);
        CYB_REQUIRE((uintptr_t)d.x % (CPLX ? 16 : 8) == 0 && (uintptr_t)d.y % (CPLX ? 16 : 8) == 0, "%s: desc %lld: misaligned pointer", who,
                    (long long)i);
        WDot w{d.x, d.y, d.rows, d.cols, d.x_rs, d.x_cs, d.y_rs, d.y_cs, d.w, 0, 0};
        auto contiguous = [&](int64_t rs, int64_t cs) { return (cs == 1 || d.cols == 1) && (rs == d.cols || d.rows == 1); };
        w.flat = contiguous(d.x_rs, d.x_cs) && (!d.y || contiguous(d.y_rs, d.y_cs));
        hd.push_back(w);
        totals.push_back(total);
    }
    if (hd.empty()) {
        CYB_HIP(hipMemsetAsync(result_dev, 0, sizeof(double) * C, ctx->stream));
        return CYB_OK;
    }
    std::vector<Item> items;
    CYB_CUT(who, items, totals, chunk_real(sum_of(totals)));
    // (the upload comes before the workspace, as in the reductions of blockops.hip)
    return with_arrays(ctx, who, items.size(), arrays(hd, items), [&](dim3 grid, const WDot* d_descs, const Item* d_items) {
        return two_stage<C, Sum>(ctx, items.size(), nullptr, 1, result_dev, [&](double* partial) {
            hipLaunchKernelGGL(wdot_stage1_kernel<CPLX>, grid, dim3(NT), 0, ctx->stream, d_descs, d_items, partial, conj_x);
            return CYB_OK;
        });
    });
}

} // namespace

extern "C" {

int cyb_tree_axis_f64(cyb_ctx_t ctx, const cyb_tree_axis_rec* recs, int64_t n, const cyb_tree_fill* fills, int64_t n_fills)
{
    return tree_axis<double>(ctx, recs, n, fills, n_fills, "cyb_tree_axis_f64");
}

int cyb_tree_axis_c128(cyb_ctx_t ctx, const cyb_tree_axis_rec* recs, int64_t n, const cyb_tree_fill* fills, int64_t n_fills)
{
    return tree_axis<d2>(ctx, recs, n, fills, n_fills, "cyb_tree_axis_c128");
}

int cyb_dot_weighted_f64(cyb_ctx_t ctx, const cyb_wdot_desc* descs, int64_t n, double* result_dev)
{
    return dot_weighted<false>(ctx, descs, n, 0, result_dev, "cyb_dot_weighted_f64");
}

int cyb_dot_weighted_c128(cyb_ctx_t ctx, const cyb_wdot_desc* descs, int64_t n, int32_t conj_x, double* result_dev)
{
    return dot_weighted<true>(ctx, descs, n, conj_x ? 1 : 0, result_dev, "cyb_dot_weighted_c128");
}

} // extern "C"
