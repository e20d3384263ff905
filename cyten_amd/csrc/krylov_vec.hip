// Vector kernels of the Krylov solvers on complex vectors (gfx950).
//
// cyb_dot_batched_c128: the inner product sum_i conj(x_i) y_i of a list of interleaved complex vectors -- the
// `inner` of the complex Krylov recurrences (Lanczos / Arnoldi on complex128 pools, krylov_based.cpp:563-589,
// 855-870) and of HipBlockBackend.inner_many on complex block lists (abelian.cpp:2159-2211).  One pass over both
// operands with 16-byte accesses; the deterministic two-stage reduction of flat_items.h, which the float64 reductions of
// blockops.hip run too (fixed work items per list, fixed summation order, no float atomics): bit-identical from run to run.
#include "flat_items.h"

#include <algorithm>

namespace {

using namespace cyb_flat; // Item, NT, chunk_complex, cut, launch, the fixed-order reduction

struct CVecDev {
    const double* x;
    const double* y;
    int64_t n;
};

// partial[2 * blockIdx.x + {0, 1}] = (re, im) of sum over the item of conj(x) y
__device__ __forceinline__ void cdot_stage1_body(const CVecDev& d, const Item& it, double* __restrict__ partial)
{
    __shared__ double red[2][WAVES];
    const GLOBAL_AS d2* x = (const GLOBAL_AS d2*)d.x + it.start;
    const GLOBAL_AS d2* y = (const GLOBAL_AS d2*)d.y + it.start;
    // two independent accumulator pairs: two 16-byte loads of each operand in flight per lane
    double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
    int64_t i = threadIdx.x;
    for (; i + NT < it.count; i += 2 * NT) {
        const d2 a = x[i], b = y[i], a1 = x[i + NT], b1 = y[i + NT];
        re0 += a.x * b.x + a.y * b.y;
        im0 += a.x * b.y - a.y * b.x;
        re1 += a1.x * b1.x + a1.y * b1.y;
        im1 += a1.x * b1.y - a1.y * b1.x;
    }
    if (i < it.count) {
        const d2 a = x[i], b = y[i];
        re0 += a.x * b.x + a.y * b.y;
        im0 += a.x * b.y - a.y * b.x;
    }
    double acc[2] = {re0 + re1, im0 + im1};
    block_reduce<2>(acc, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = acc[0];
        partial[2 * blockIdx.x + 1] = acc[1];
    }
}

__global__ void __launch_bounds__(NT) cdot_stage1_kernel(const CVecDev* __restrict__ descs, const Item* __restrict__ items,
                                                         double* __restrict__ partial)
{
    const Item it = items[blockIdx.x];
    cdot_stage1_body(descs[it.desc], it, partial);
}

// ONE vector: descriptor and chunking travel as kernel arguments (no descriptor upload) -- every inner product of the
// Krylov recurrences on flat pools is of this kind
__global__ void __launch_bounds__(NT) cdot_stage1_one_kernel(CVecDev d, int64_t chunk, double* __restrict__ partial)
{
    cdot_stage1_body(d, nth_item(chunk, d.n), partial);
}

} // namespace

extern "C" {

int cyb_dot_batched_c128(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev)
{
    CYB_REQUIRE(ctx && result_dev, "cyb_dot_batched_c128: NULL argument");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "cyb_dot_batched_c128: bad descriptor list");
    const char* who = "cyb_dot_batched_c128";
    std::vector<CVecDev> hv((size_t)n);
    std::vector<int64_t> totals((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        CYB_REQUIRE(descs[i].n >= 0, "cyb_dot_batched_c128: desc %lld: negative length", (long long)i);
        CYB_REQUIRE(descs[i].n == 0 || (descs[i].x && descs[i].y), "cyb_dot_batched_c128: desc %lld: NULL operand", (long long)i);
        hv[(size_t)i] = CVecDev{descs[i].x, descs[i].y, descs[i].n};
        totals[(size_t)i] = descs[i].n;
    }
    const int64_t total = sum_of(totals), chunk = chunk_complex(total);
    if (n == 1 && total > 0) { // ONE vector: no descriptor upload
        const int64_t n_items = cdiv64(total, chunk);
        return two_stage<2, Sum>(ctx, (size_t)n_items, nullptr, 1, result_dev, [&](double* partial) {
            hipLaunchKernelGGL(cdot_stage1_one_kernel, dim3((unsigned)n_items), dim3(NT), 0, ctx->stream, hv[0], chunk, partial);
            return CYB_OK;
        });
    }
    std::vector<Item> items;
    CYB_CUT(who, items, totals, chunk);
    return two_stage<2, Sum>(ctx, items.size(), nullptr, 1, result_dev,
                             [&](double* partial) { return launch(ctx, who, cdot_stage1_kernel, arrays(hv, items), partial); });
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// Projections against a list of basis vectors: multi-dot, multi-axpy and the fused classical Gram-Schmidt step of GMRES
// (krylov_based.cpp:453-469) and of the projected operator (sparse.cpp:294-327).
//
// One kernel template serves all three.  The grid and the row range of every workgroup depend on (n, m) only: workgroup g
// owns the tiles [g * tpg, (g + 1) * tpg) of TS = 64 * EL elements.  Inside a tile the four waves split the basis (wave q
// takes j = q, q + 4, ...) and hold their V rows in registers, so the update w + alpha sum_j h_j V_j (summed per wave, then
// over the waves in a fixed order through LDS) and the partial dots of the updated w read V from HBM once.  Partials go to
// a (workgroup, j) table that a second kernel sums in a fixed order: no float atomics, bit-identical from run to run.
// CGS with passes = 2 is three such sweeps, dot / update+dot / update+norm: (3m + 5) n words.
namespace {

constexpr int GS_MAX_M = 64;
constexpr int GS_WAVES = 4;
constexpr int GS_MAX_GRID = 2048;
constexpr int GS_GRANULE = 256; // elements (doubles or complex numbers) per entry of a weight table

struct BasisPtrs {
    const double* v[GS_MAX_M];
};

enum GsMode : int { GS_DOT = 0, GS_UPD_DOT = 1, GS_UPD_NORM = 2, GS_UPD = 3 };

template <bool CPLX> struct GsT;
template <> struct GsT<false> {
    typedef double T;
    static constexpr int EL = 4;
    static __device__ __forceinline__ T zero() { return 0.0; }
    static __device__ __forceinline__ void cdot(T v, T w, double& re, double&) { re += v * w; }
    static __device__ __forceinline__ T madd(T acc, double hre, double, T v) { return acc + hre * v; }
    static __device__ __forceinline__ T scale(double are, double, T u) { return are * u; }
    static __device__ __forceinline__ double sq(T w) { return w * w; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
    static __device__ __forceinline__ T wscale(double d, T w) { return d * w; }
    static __device__ __forceinline__ double sqw(T wd, T w) { return wd * w; }
};
template <> struct GsT<true> {
    typedef d2 T;
    static constexpr int EL = 2;
    static __device__ __forceinline__ T zero() { return T{0.0, 0.0}; }
    static __device__ __forceinline__ void cdot(T v, T w, double& re, double& im)
    {
        re += v.x * w.x + v.y * w.y;
        im += v.x * w.y - v.y * w.x;
    }
    static __device__ __forceinline__ T madd(T acc, double hre, double him, T v)
    {
        return T{acc.x + (hre * v.x - him * v.y), acc.y + (hre * v.y + him * v.x)};
    }
    static __device__ __forceinline__ T scale(double are, double aim, T u) { return T{are * u.x - aim * u.y, are * u.y + aim * u.x}; }
    static __device__ __forceinline__ double sq(T w) { return w.x * w.x + w.y * w.y; }
    static __device__ __forceinline__ T add(T a, T b) { return T{a.x + b.x, a.y + b.y}; }
    static __device__ __forceinline__ T wscale(double d, T w) { return T{d * w.x, d * w.y}; }
    static __device__ __forceinline__ double sqw(T wd, T w) { return wd.x * w.x + wd.y * w.y; }
};

// partial[(g * (m + 1) + j) * 2 + {0, 1}]: (re, im) of the workgroup's partial dot with V_j (j < m) or its partial |w|^2
// (j == m).  coef: m (real) or 2m (interleaved complex) device doubles, scaled by alpha in the update.
//
// WT: the reductions carry a weight per granule of GS_GRANULE elements (the quantum dimension of the coupled sector a
// fusion-tree pool keeps there): h_j = sum_i d(i) conj(V_j[i]) w[i], |w|^2 = sum_i d(i) |w[i]|^2; the update is unweighted.
// A tile is one granule (f64) or half of one (c128), so the weight is uniform per tile: it is read once per tile and
// multiplied onto the tile's EL elements of w before they meet the J rows of V -- EL multiplications per lane and tile,
// whatever J is, and the accumulation chain of every lane is the unweighted one term for term (a weight d = s^2 with s a
// power of two therefore gives the bits of the unweighted kernel on (s V, s w)).
template <bool CPLX, int J, int MODE, bool WT>
__global__ void __launch_bounds__(64 * GS_WAVES) gs_sweep_kernel(BasisPtrs P, int m, double* __restrict__ w_, int64_t n, int64_t tpg,
                                                                const double* __restrict__ coef, double are, double aim,
                                                                double* __restrict__ partial, const double* __restrict__ weights)
{
    typedef GsT<CPLX> O;
    typedef typename O::T T;
    constexpr int EL = O::EL;
    constexpr int TS = 64 * EL;
    constexpr bool UPD = MODE != GS_DOT;
    constexpr bool DOT = MODE == GS_DOT || MODE == GS_UPD_DOT;
    __shared__ T red[GS_WAVES][EL][64];
    T* __restrict__ w = reinterpret_cast<T*>(w_);
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double hre[J], him[J], dre[J], dim[J];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
        const int j = q + GS_WAVES * jj;
        hre[jj] = him[jj] = dre[jj] = dim[jj] = 0.0;
        if (UPD && j < m) {
            hre[jj] = CPLX ? coef[2 * j] : coef[j];
            him[jj] = CPLX ? coef[2 * j + 1] : 0.0;
        }
    }
    double nrm = 0.0;
    const int64_t t_end = min(((int64_t)blockIdx.x + 1) * tpg, (n + TS - 1) / TS);
    for (int64_t t = (int64_t)blockIdx.x * tpg; t < t_end; ++t) {
        const int64_t base = t * TS + lane;
        T vr[J][EL];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
            const int j = q + GS_WAVES * jj;
            const T* __restrict__ v = reinterpret_cast<const T*>(j < m ? P.v[j] : nullptr);
#pragma unroll
            for (int e = 0; e < EL; ++e) {
                const int64_t i = base + 64 * e;
                vr[jj][e] = (j < m && i < n) ? v[i] : O::zero();
            }
        }
        T wr[EL];
#pragma unroll
        for (int e = 0; e < EL; ++e) {
            const int64_t i = base + 64 * e;
            wr[e] = i < n ? w[i] : O::zero();
        }
        if (UPD) {
#pragma unroll
            for (int e = 0; e < EL; ++e) {
                T u = O::zero();
#pragma unroll
                for (int jj = 0; jj < J; ++jj) u = O::madd(u, hre[jj], him[jj], vr[jj][e]);
                red[q][e][lane] = u;
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < EL; ++e) {
                const T u = O::add(O::add(red[0][e][lane], red[1][e][lane]), O::add(red[2][e][lane], red[3][e][lane]));
                wr[e] = O::add(wr[e], O::scale(are, aim, u));
                const int64_t i = base + 64 * e;
                if (q == 0 && i < n) w[i] = wr[e];
            }
            __syncthreads(); // (red is refilled by the next tile)
        }
        if (WT) {
            static_assert(GS_GRANULE % TS == 0, "a tile must not straddle a granule");
            const double d = weights[t / (GS_GRANULE / TS)];
            T wd[EL];
#pragma unroll
            for (int e = 0; e < EL; ++e) wd[e] = O::wscale(d, wr[e]);
            if (DOT) {
#pragma unroll
                for (int jj = 0; jj < J; ++jj)
#pragma unroll
                    for (int e = 0; e < EL; ++e) O::cdot(vr[jj][e], wd[e], dre[jj], dim[jj]);
            }
            if (MODE == GS_UPD_NORM && q == 0) {
#pragma unroll
                for (int e = 0; e < EL; ++e) nrm += O::sqw(wd[e], wr[e]);
            }
            continue;
        }
        if (DOT) {
#pragma unroll
            for (int jj = 0; jj < J; ++jj)
#pragma unroll
                for (int e = 0; e < EL; ++e) O::cdot(vr[jj][e], wr[e], dre[jj], dim[jj]);
        }
        if (MODE == GS_UPD_NORM && q == 0) {
#pragma unroll
            for (int e = 0; e < EL; ++e) nrm += O::sq(wr[e]);
        }
    }
    double* out = partial + (int64_t)blockIdx.x * (m + 1) * 2;
    if (DOT) {
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
            const int j = q + GS_WAVES * jj;
            const double r = wave_sum(dre[jj]);
            const double s = CPLX ? wave_sum(dim[jj]) : 0.0;
            if (lane == 0 && j < m) {
                out[2 * j] = r;
                out[2 * j + 1] = s;
            }
        }
    }
    if (MODE == GS_UPD_NORM && q == 0) {
        const double r = wave_sum(nrm);
        if (lane == 0) {
            out[2 * m] = r;
            out[2 * m + 1] = 0.0;
        }
    }
}

// Sums the partial table over the n_groups workgroups in a fixed order, one workgroup per column c in [c0, c0 + gridDim.x).
// Columns j < m: coef_out[j] = the sum (the coefficients of the next sweep) and, with `add`, sum_out[j] = add[j] + sum (the
// CGS2 coefficients of both passes); real results take one double each, complex two.  Column m: norm_out = sqrt(sum).
__global__ void __launch_bounds__(NT) gs_reduce_kernel(const double* __restrict__ partial, int64_t n_groups, int m, int cplx, int c0,
                                                       double* __restrict__ coef_out, const double* __restrict__ add,
                                                       double* __restrict__ sum_out, double* __restrict__ norm_out)
{
    __shared__ double red[2][WAVES];
    const int c = c0 + blockIdx.x;
    double acc[2];
    reduce_rows<2, Sum>(acc, partial, 0, n_groups, m + 1, c, red);
    if (threadIdx.x != 0) return;
    const double r = acc[0], s = acc[1];
    if (c == m) {
        norm_out[0] = sqrt(r);
        return;
    }
    if (cplx) {
        if (coef_out) {
            coef_out[2 * c] = r;
            coef_out[2 * c + 1] = s;
        }
        if (add) {
            sum_out[2 * c] = add[2 * c] + r;
            sum_out[2 * c + 1] = add[2 * c + 1] + s;
        }
    } else {
        if (coef_out) coef_out[c] = r;
        if (add) sum_out[c] = add[c] + r;
    }
}

struct GsGrid {
    int64_t groups, tpg;
};

static GsGrid gs_grid(int64_t n, bool cplx)
{
    const int64_t ts = 64 * (cplx ? GsT<true>::EL : GsT<false>::EL);
    const int64_t tiles = cdiv64(n, ts);
    const int64_t tpg = std::max<int64_t>(1, cdiv64(tiles, GS_MAX_GRID));
    return GsGrid{cdiv64(tiles, tpg), tpg};
}

template <bool CPLX, int MODE, bool WT>
static void gs_launch_j(int J, const GsGrid& g, hipStream_t s, const BasisPtrs& P, int m, double* w, int64_t n, const double* coef,
                        double are, double aim, double* partial, const double* weights)
{
    const dim3 grid((unsigned)g.groups), block(64 * GS_WAVES);
#define GS_CASE(JJ)                                                                                                    \
    case JJ: hipLaunchKernelGGL((gs_sweep_kernel<CPLX, JJ, MODE, WT>), grid, block, 0, s, P, m, w, n, g.tpg, coef, are, aim, partial, weights); break;
    switch (J) {
        GS_CASE(1)
        GS_CASE(2)
        GS_CASE(4)
        GS_CASE(8)
        default: GS_CASE(16)
    }
#undef GS_CASE
}

// `weights` (a granule table, or nullptr: the unweighted instantiations) only reaches the sweeps that reduce
template <bool CPLX>
static void gs_sweep(int mode, const GsGrid& g, hipStream_t s, const BasisPtrs& P, int m, double* w, int64_t n, const double* coef,
                     double are, double aim, double* partial, const double* weights = nullptr)
{
    if (g.groups == 0) return;
    int J = 1;
    while (J * GS_WAVES < m) J *= 2;
    if (weights) {
        switch (mode) {
        case GS_DOT: gs_launch_j<CPLX, GS_DOT, true>(J, g, s, P, m, w, n, coef, are, aim, partial, weights); break;
        case GS_UPD_DOT: gs_launch_j<CPLX, GS_UPD_DOT, true>(J, g, s, P, m, w, n, coef, are, aim, partial, weights); break;
        default: gs_launch_j<CPLX, GS_UPD_NORM, true>(J, g, s, P, m, w, n, coef, are, aim, partial, weights); break;
        }
        return;
    }
    switch (mode) {
    case GS_DOT: gs_launch_j<CPLX, GS_DOT, false>(J, g, s, P, m, w, n, coef, are, aim, partial, nullptr); break;
    case GS_UPD_DOT: gs_launch_j<CPLX, GS_UPD_DOT, false>(J, g, s, P, m, w, n, coef, are, aim, partial, nullptr); break;
    case GS_UPD_NORM: gs_launch_j<CPLX, GS_UPD_NORM, false>(J, g, s, P, m, w, n, coef, are, aim, partial, nullptr); break;
    default: gs_launch_j<CPLX, GS_UPD, false>(J, g, s, P, m, w, n, coef, are, aim, partial, nullptr); break;
    }
}

static int gs_args(const char* fn, const double* const* basis, int64_t m, const void* w, int64_t n, bool cplx, BasisPtrs* P)
{
    if (m > GS_MAX_M) {
        cyb::set_error("%s: %lld basis vectors, at most %d are supported", fn, (long long)m, GS_MAX_M);
        return CYB_ERR_UNSUPPORTED;
    }
    CYB_REQUIRE(m >= 0 && n >= 0, "%s: negative size", fn);
    CYB_REQUIRE(m == 0 || basis, "%s: NULL basis list", fn);
    const uintptr_t align = cplx ? 16 : 8;
    CYB_REQUIRE(n == 0 || (w && (uintptr_t)w % align == 0), "%s: NULL or misaligned vector", fn);
    for (int64_t j = 0; j < m; ++j) {
        CYB_REQUIRE(n == 0 || (basis[j] && (uintptr_t)basis[j] % align == 0), "%s: basis vector %lld NULL or misaligned", fn, (long long)j);
        P->v[j] = basis[j];
    }
    for (int64_t j = m; j < GS_MAX_M; ++j) P->v[j] = nullptr;
    return CYB_OK;
}

// the granule table of a weighted entry: ceil(n / GS_GRANULE) device doubles
static int gs_weights(const char* fn, bool weighted, const double* wt, int64_t n)
{
    CYB_REQUIRE(!weighted || n == 0 || (wt && (uintptr_t)wt % 8 == 0), "%s: NULL or misaligned weight table", fn);
    return CYB_OK;
}

// partial table of one sweep + (for CGS2) the pass-1 and pass-2 coefficients, in workspace slot 0
static int gs_workspace(cyb_ctx_t ctx, const GsGrid& g, int64_t m, double** partial, double** h1, double** h2)
{
    const size_t np = (size_t)std::max<int64_t>(g.groups, 1) * (size_t)(m + 1) * 2;
    void* ws = nullptr;
    CYB_TRY(ctx->workspace(sizeof(double) * (np + 4 * GS_MAX_M), &ws));
    *partial = static_cast<double*>(ws);
    *h1 = *partial + np;
    *h2 = *h1 + 2 * GS_MAX_M;
    return CYB_OK;
}

template <bool CPLX>
static int gram_schmidt(const char* fn, cyb_ctx_t ctx, const double* const* basis, int64_t m, double* w, int64_t n, int32_t passes,
                        double* out_dev, bool weighted = false, const double* wt = nullptr)
{
    CYB_REQUIRE(ctx && out_dev, "%s: NULL argument", fn);
    BasisPtrs P;
    CYB_TRY(gs_args(fn, basis, m, w, n, CPLX, &P));
    CYB_TRY(gs_weights(fn, weighted, wt, n));
    CYB_REQUIRE(passes == 1 || passes == 2, "%s: passes must be 1 or 2, got %d", fn, (int)passes);
    const GsGrid g = gs_grid(n, CPLX);
    double *partial, *h1, *h2;
    CYB_TRY(gs_workspace(ctx, g, m, &partial, &h1, &h2));
    const int mi = (int)m, c = CPLX ? 1 : 0;
    const hipStream_t s = ctx->stream;
    double* norm_out = out_dev + (CPLX ? 2 : 1) * m;
    // pass 1: h1 = V^H w (straight into out_dev for one pass)
    double* hp1 = passes == 1 ? out_dev : h1;
    if (m > 0) {
        gs_sweep<CPLX>(GS_DOT, g, s, P, mi, w, n, nullptr, 0.0, 0.0, partial, wt);
        hipLaunchKernelGGL(gs_reduce_kernel, dim3((unsigned)m), dim3(NT), 0, s, partial, g.groups, mi, c, 0, hp1, nullptr, nullptr, nullptr);
    }
    const double* last = hp1;
    if (passes == 2 && m > 0) { // w -= V h1, h2 = V^H w; out = h1 + h2
        gs_sweep<CPLX>(GS_UPD_DOT, g, s, P, mi, w, n, hp1, -1.0, 0.0, partial, wt);
        hipLaunchKernelGGL(gs_reduce_kernel, dim3((unsigned)m), dim3(NT), 0, s, partial, g.groups, mi, c, 0, h2, hp1, out_dev, nullptr);
        last = h2;
    }
    // w -= V h_last, |w|
    gs_sweep<CPLX>(GS_UPD_NORM, g, s, P, mi, w, n, m > 0 ? last : nullptr, -1.0, 0.0, partial, wt);
    hipLaunchKernelGGL(gs_reduce_kernel, dim3(1), dim3(NT), 0, s, partial, g.groups, mi, c, mi, nullptr, nullptr, nullptr, norm_out);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

template <bool CPLX>
static int multi_dot(const char* fn, cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* w, int64_t n, double* h_dev,
                     bool weighted = false, const double* wt = nullptr)
{
    CYB_REQUIRE(ctx && (m == 0 || h_dev), "%s: NULL argument", fn);
    BasisPtrs P;
    CYB_TRY(gs_args(fn, basis, m, w, n, CPLX, &P));
    CYB_TRY(gs_weights(fn, weighted, wt, n));
    if (m == 0) return CYB_OK;
    const GsGrid g = gs_grid(n, CPLX);
    double *partial, *h1, *h2;
    CYB_TRY(gs_workspace(ctx, g, m, &partial, &h1, &h2));
    gs_sweep<CPLX>(GS_DOT, g, ctx->stream, P, (int)m, const_cast<double*>(w), n, nullptr, 0.0, 0.0, partial, wt);
    hipLaunchKernelGGL(gs_reduce_kernel, dim3((unsigned)m), dim3(NT), 0, ctx->stream, partial, g.groups, (int)m, CPLX ? 1 : 0, 0, h_dev,
                       nullptr, nullptr, nullptr);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

template <bool CPLX>
static int multi_axpy(const char* fn, cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* h_dev, double are, double aim,
                      double* w, int64_t n)
{
    CYB_REQUIRE(ctx && (m == 0 || n == 0 || h_dev), "%s: NULL argument", fn);
    BasisPtrs P;
    CYB_TRY(gs_args(fn, basis, m, w, n, CPLX, &P));
    if (m == 0 || n == 0) return CYB_OK;
    const GsGrid g = gs_grid(n, CPLX);
    gs_sweep<CPLX>(GS_UPD, g, ctx->stream, P, (int)m, w, n, h_dev, are, aim, nullptr);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Orthonormalising a LIST of vectors (gram_schmidt(vecs, rcond), sparse.cpp:420-436) without a host wait between its steps:
// step k is the CGS2 sequence above of vecs[k] against vecs[0..k-1], then the kernel below, which reads the norm that
// sequence left on the device and either scales the vector by 1 / norm or WRITES zeros over it.  A dropped vector is then
// all +0.0 bytes whatever it held (NaN, Inf): as a basis vector of the later steps its coefficient is a sum of zeros and its
// share of every update is a zero, so the list runs on without the host knowing which vectors were dropped.
//
// The vector is a range of `words` doubles (a complex vector: 2n of them, both parts take the same factor), cut into items by
// the cutter of flat_items.h; one pass, 2 words moved per element.  An item starts at an even word (chunks are multiples of
// 1024), so after at most one leading word -- an f64 vector that is only 8-byte aligned -- every access is 16 bytes wide.
__global__ void __launch_bounds__(NT) normalize_or_zero_kernel(const Item* __restrict__ items, double* __restrict__ x_,
                                                                const double* __restrict__ norm_dev, double rcond,
                                                                double* __restrict__ norm_out, double* __restrict__ flag_out)
{
    const Item it = items[blockIdx.x];
    const double norm = norm_dev[0];
    const bool keep = norm > rcond; // false for a NaN norm
    const double f = 1.0 / norm;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        norm_out[0] = norm;
        flag_out[0] = keep ? 1.0 : 0.0;
    }
    gp x = (gp)x_ + it.start;
    const int64_t head = min(it.count, (int64_t)(((uintptr_t)x >> 3) & 1));
    const int64_t nv = (it.count - head) / 2;
    if (threadIdx.x == 0 && head) x[0] = keep ? x[0] * f : 0.0;
    GLOBAL_AS d2* xv = (GLOBAL_AS d2*)(x + head);
    if (keep) {
        for (int64_t i = threadIdx.x; i < nv; i += NT) {
            const d2 a = xv[i];
            xv[i] = d2{a.x * f, a.y * f};
        }
    } else {
        for (int64_t i = threadIdx.x; i < nv; i += NT) xv[i] = d2{0.0, 0.0};
    }
    const int64_t tail = head + 2 * nv;
    if (threadIdx.x == 0 && tail < it.count) x[tail] = keep ? x[tail] * f : 0.0;
}

template <bool CPLX>
static int orthonormalize(const char* fn, cyb_ctx_t ctx, double* const* vecs, int64_t m, int64_t n, double rcond, double* out_dev,
                          bool weighted = false, const double* wt = nullptr)
{
    CYB_REQUIRE(ctx, "%s: NULL argument", fn);
    BasisPtrs P;
    CYB_TRY(gs_args(fn, vecs, m, (m > 0 && vecs) ? vecs[0] : nullptr, m > 0 ? n : 0, CPLX, &P));
    CYB_TRY(gs_weights(fn, weighted, wt, n));
    if (m == 0 || n == 0) return CYB_OK;
    CYB_REQUIRE(out_dev && (uintptr_t)out_dev % 8 == 0, "%s: NULL or misaligned out_dev", fn);
    // Workspace slot 0 for the longest step at once (a slot that grows waits for the stream): the steps then find it large
    // enough.  Behind the part gram_schmidt uses, the coefficients and the norm of the current step.
    const GsGrid g = gs_grid(n, CPLX);
    const size_t np_max = (size_t)g.groups * (size_t)m * 2, gs_doubles = np_max + 4 * GS_MAX_M;
    void* ws = nullptr;
    CYB_TRY(ctx->workspace(sizeof(double) * (gs_doubles + 2 * GS_MAX_M + 1), &ws));
    double* step_out = static_cast<double*>(ws) + gs_doubles;
    const int64_t words = (CPLX ? 2 : 1) * n;
    std::vector<Item> items;
    CYB_CUT(fn, items, std::vector<int64_t>{words}, chunk_real(words));
    // ONE upload of the items for the whole list: every step cuts its vector the same way
    return with_arrays(ctx, fn, items.size(), arrays(items), [&](dim3 grid, const Item* d_items) -> int {
        for (int64_t k = 0; k < m; ++k) {
            CYB_TRY(gram_schmidt<CPLX>(fn, ctx, vecs, k, vecs[k], n, 2, step_out, weighted, wt));
            hipLaunchKernelGGL(normalize_or_zero_kernel, grid, dim3(NT), 0, ctx->stream, d_items, vecs[k],
                               step_out + (CPLX ? 2 : 1) * k, rcond, out_dev + k, out_dev + m + k);
        }
        return CYB_OK;
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// Basis rotation Y = V S of a thick restart (Wu & Simon): dst[i][p] = sum_{j < m} q[j][i] src[j][p], i < k.  One pass that
// reads the m basis vectors once and writes the k results once: (m + k) n words, against k (m + 1) n for k linear
// combinations.
//
// One thread per position (two adjacent ones, 16 bytes, when every pointer is 16-byte aligned; a pointer that is only 8-byte
// aligned sends the whole call to the 8-byte instantiation -- the same chain per position, hence the same bits).  A thread
// keeps KC accumulators per position (KC = k rounded up to 4 / 8 / 16 / 32, the columns i >= k of the uploaded matrix are
// zero and are not stored) and adds the terms with j ASCENDING, one fma each: no atomics, no reduction across threads,
// bit-identical from run to run.
//
// ALIASING: a dst[i] may be any src[j].  Every accumulator depends on all m loads of the thread's positions, so every one of
// its k stores comes after all of them (a data dependence; the pointers carry no __restrict__), and a thread reads and writes
// its own positions only: whatever a store overwrites has been read by the only thread that needs it.  Keep both properties --
// all loads of a position before its first store, no position shared between threads -- when changing this kernel.  Ranges
// that overlap only partly would break the second one; the host refuses them.
//
// The coefficients are wave-uniform: the matrix (m x KC doubles in a ring slot) is read through the constant address space,
// i.e. by scalar loads through the scalar cache into SGPRs, and enters the fma as its scalar operand.  No VGPRs, no LDS
// traffic and no barrier; LDS would cost KC / 2 ds_read_b128 per j next to KC (or 2 KC) fma.
constexpr int ROT_MAX_K = 32;

struct RotDst {
    double* v[ROT_MAX_K];
};

typedef const __attribute__((address_space(4))) double* rot_cq;

template <class T> struct RotFma;
template <> struct RotFma<double> {
    static __device__ __forceinline__ double zero() { return 0.0; }
    static __device__ __forceinline__ double fma(double c, double x, double a) { return __builtin_fma(c, x, a); }
};
template <> struct RotFma<d2> {
    static __device__ __forceinline__ d2 zero() { return d2{0.0, 0.0}; }
    static __device__ __forceinline__ d2 fma(double c, d2 x, d2 a) { return d2{__builtin_fma(c, x.x, a.x), __builtin_fma(c, x.y, a.y)}; }
};

// the positions [off, off + sizeof(T) / 8) of every vector
template <int KC, class T>
__device__ __forceinline__ void rotate_at(const BasisPtrs& S, int m, const RotDst& D, int k, rot_cq q, int64_t off)
{
    T acc[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) acc[i] = RotFma<T>::zero();
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
        const T x = *reinterpret_cast<const GLOBAL_AS T*>((gcp)S.v[j] + off);
#pragma unroll
        for (int i = 0; i < KC; ++i) acc[i] = RotFma<T>::fma(q[j * KC + i], x, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < KC; ++i)
        if (i < k) *reinterpret_cast<GLOBAL_AS T*>((gp)D.v[i] + off) = acc[i];
}

// workgroup g owns the tiles [g * tpg, (g + 1) * tpg) of NT * W positions, W = 2 (VEC) or 1
template <int KC, bool VEC>
__global__ void __launch_bounds__(NT) basis_rotate_kernel(BasisPtrs S, int m, RotDst D, int k, const double* q_, int64_t n, int64_t tpg)
{
    constexpr int W = VEC ? 2 : 1;
    constexpr int64_t TS = (int64_t)NT * W;
    const rot_cq q = (rot_cq)q_;
    const int64_t t_end = min(((int64_t)blockIdx.x + 1) * tpg, (n + TS - 1) / TS);
    for (int64_t t = (int64_t)blockIdx.x * tpg; t < t_end; ++t) {
        const int64_t off = t * TS + (int64_t)threadIdx.x * W;
        if (VEC && off + 1 < n)
            rotate_at<KC, d2>(S, m, D, k, q, off);
        else if (off < n) // (VEC: the last position of an odd n)
            rotate_at<KC, double>(S, m, D, k, q, off);
    }
}

template <bool VEC>
static void rot_launch(int KC, dim3 grid, hipStream_t s, const BasisPtrs& S, int m, const RotDst& D, int k, const double* q, int64_t n,
                       int64_t tpg)
{
#define ROT_CASE(KK)                                                                                                   \
    case KK: hipLaunchKernelGGL((basis_rotate_kernel<KK, VEC>), grid, dim3(NT), 0, s, S, m, D, k, q, n, tpg); break;
    switch (KC) {
        ROT_CASE(4)
        ROT_CASE(8)
        ROT_CASE(16)
        default: ROT_CASE(32)
    }
#undef ROT_CASE
}

static int basis_rotate(const char* fn, cyb_ctx_t ctx, const double* const* src, int64_t m, double* const* dst, int64_t k,
                        const double* q_host, int64_t n)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", fn);
    CYB_REQUIRE(m >= 0 && k >= 0 && n >= 0, "%s: negative size", fn);
    CYB_REQUIRE(m <= GS_MAX_M, "%s: %lld basis vectors, at most %d are supported", fn, (long long)m, GS_MAX_M);
    CYB_REQUIRE(k <= ROT_MAX_K, "%s: %lld columns, at most %d are supported (split the columns)", fn, (long long)k, ROT_MAX_K);
    if (m == 0 || k == 0 || n == 0) return CYB_OK;
    CYB_REQUIRE(src && dst && q_host, "%s: NULL table", fn);
    CYB_REQUIRE(n <= (INT64_MAX >> 4), "%s: vector too long", fn);
    BasisPtrs S;
    RotDst D;
    uintptr_t bits = 0;
    for (int64_t j = 0; j < GS_MAX_M; ++j) {
        S.v[j] = j < m ? src[j] : nullptr;
        CYB_REQUIRE(j >= m || (src[j] && (uintptr_t)src[j] % 8 == 0), "%s: src %lld NULL or misaligned", fn, (long long)j);
        bits |= (uintptr_t)S.v[j];
    }
    for (int64_t i = 0; i < ROT_MAX_K; ++i) {
        D.v[i] = i < k ? dst[i] : nullptr;
        CYB_REQUIRE(i >= k || (dst[i] && (uintptr_t)dst[i] % 8 == 0), "%s: dst %lld NULL or misaligned", fn, (long long)i);
        bits |= (uintptr_t)D.v[i];
    }
    // a dst range is disjoint from every other dst range, and from every src range unless it IS that range
    const uintptr_t len = (uintptr_t)n * sizeof(double);
    const auto overlap = [len](const void* a, const void* b) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return x < y + len && y < x + len;
    };
    for (int64_t i = 0; i < k; ++i) {
        for (int64_t i2 = 0; i2 < i; ++i2)
            CYB_REQUIRE(!overlap(dst[i], dst[i2]), "%s: dst %lld and dst %lld are equal or overlap", fn, (long long)i2, (long long)i);
        for (int64_t j = 0; j < m; ++j)
            CYB_REQUIRE(dst[i] == src[j] || !overlap(dst[i], src[j]), "%s: dst %lld overlaps src %lld partly", fn, (long long)i,
                        (long long)j);
    }
    int KC = 4;
    while (KC < k) KC *= 2;
    std::vector<double> qp((size_t)m * KC, 0.0); // columns k .. KC - 1 are zero
    for (int64_t j = 0; j < m; ++j) std::copy(q_host + j * k, q_host + (j + 1) * k, qp.begin() + j * KC);
    void* q_dev = nullptr;
    CYB_TRY(cyb::upload_packed(ctx, {{qp.data(), sizeof(double) * qp.size(), &q_dev}}));
    const bool vec = bits % 16 == 0;
    const int64_t tiles = cdiv64(n, (int64_t)NT * (vec ? 2 : 1));
    const int64_t tpg = std::max<int64_t>(1, cdiv64(tiles, GS_MAX_GRID));
    const dim3 grid((unsigned)cdiv64(tiles, tpg));
    if (vec)
        rot_launch<true>(KC, grid, ctx->stream, S, (int)m, D, (int)k, static_cast<const double*>(q_dev), n, tpg);
    else
        rot_launch<false>(KC, grid, ctx->stream, S, (int)m, D, (int)k, static_cast<const double*>(q_dev), n, tpg);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

} // namespace

extern "C" {

int cyb_basis_rotate_f64(cyb_ctx_t ctx, const double* const* src, int64_t m, double* const* dst, int64_t k, const double* q_host, int64_t n)
{
    return basis_rotate("cyb_basis_rotate_f64", ctx, src, m, dst, k, q_host, n);
}

int cyb_orthonormalize_f64(cyb_ctx_t ctx, double* const* vecs, int64_t m, int64_t n, double rcond, double* out_dev)
{
    return orthonormalize<false>("cyb_orthonormalize_f64", ctx, vecs, m, n, rcond, out_dev);
}

int cyb_orthonormalize_c128(cyb_ctx_t ctx, double* const* vecs, int64_t m, int64_t n, double rcond, double* out_dev)
{
    return orthonormalize<true>("cyb_orthonormalize_c128", ctx, vecs, m, n, rcond, out_dev);
}

int cyb_orthonormalize_weighted_f64(cyb_ctx_t ctx, double* const* vecs, int64_t m, int64_t n, double rcond, const double* weights_dev,
                                    double* out_dev)
{
    return orthonormalize<false>("cyb_orthonormalize_weighted_f64", ctx, vecs, m, n, rcond, out_dev, true, weights_dev);
}

int cyb_orthonormalize_weighted_c128(cyb_ctx_t ctx, double* const* vecs, int64_t m, int64_t n, double rcond, const double* weights_dev,
                                     double* out_dev)
{
    return orthonormalize<true>("cyb_orthonormalize_weighted_c128", ctx, vecs, m, n, rcond, out_dev, true, weights_dev);
}

int cyb_gram_schmidt_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, double* w, int64_t n, int32_t passes, double* out_dev)
{
    return gram_schmidt<false>("cyb_gram_schmidt_f64", ctx, basis, m, w, n, passes, out_dev);
}

int cyb_gram_schmidt_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, double* w, int64_t n, int32_t passes, double* out_dev)
{
    return gram_schmidt<true>("cyb_gram_schmidt_c128", ctx, basis, m, w, n, passes, out_dev);
}

int cyb_multi_dot_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* w, int64_t n, double* h_dev)
{
    return multi_dot<false>("cyb_multi_dot_f64", ctx, basis, m, w, n, h_dev);
}

int cyb_multi_dot_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* w, int64_t n, double* h_dev)
{
    return multi_dot<true>("cyb_multi_dot_c128", ctx, basis, m, w, n, h_dev);
}

int cyb_multi_dot_weighted_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* w, int64_t n, const double* weights_dev,
                               double* h_dev)
{
    return multi_dot<false>("cyb_multi_dot_weighted_f64", ctx, basis, m, w, n, h_dev, true, weights_dev);
}

int cyb_multi_dot_weighted_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* w, int64_t n, const double* weights_dev,
                                double* h_dev)
{
    return multi_dot<true>("cyb_multi_dot_weighted_c128", ctx, basis, m, w, n, h_dev, true, weights_dev);
}

int cyb_gram_schmidt_weighted_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, double* w, int64_t n, int32_t passes,
                                  const double* weights_dev, double* out_dev)
{
    return gram_schmidt<false>("cyb_gram_schmidt_weighted_f64", ctx, basis, m, w, n, passes, out_dev, true, weights_dev);
}

int cyb_gram_schmidt_weighted_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, double* w, int64_t n, int32_t passes,
                                   const double* weights_dev, double* out_dev)
{
    return gram_schmidt<true>("cyb_gram_schmidt_weighted_c128", ctx, basis, m, w, n, passes, out_dev, true, weights_dev);
}

int cyb_multi_axpy_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* h_dev, double alpha, double* w, int64_t n)
{
    return multi_axpy<false>("cyb_multi_axpy_f64", ctx, basis, m, h_dev, alpha, 0.0, w, n);
}

int cyb_multi_axpy_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* h_dev, double alpha_re, double alpha_im,
                        double* w, int64_t n)
{
    return multi_axpy<true>("cyb_multi_axpy_c128", ctx, basis, m, h_dev, alpha_re, alpha_im, w, n);
}

} // extern "C"
