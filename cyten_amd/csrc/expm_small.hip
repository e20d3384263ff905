// Grouped matrix exponential of small blocks: E = exp(alpha * A) for every listed matrix in ONE launch, one workgroup per
// matrix, the whole computation out of LDS.
//
// NumpyBlockBackend::matrix_exp = scipy.linalg.expm (src/block_backend/numpy.cpp:1227-1234) is called once per diagonal block
// by AbelianBackend::act_block_diagonal_square_matrix (src/backends/abelian.cpp:562-593).  The algorithm is the one
// HipBlockBackend.matrix_exp runs with one launch per step: 1-norm of alpha * A, s = 0 if it is <= 1/2 else
// ceil(log2(norm / (1/2))), the degree-18 Taylor polynomial of M = alpha * A / 2^s in Horner form P <- I + (M / k) P for
// k = 18 .. 1, then s squarings.  ||M||_1 <= 1/2 makes the truncation error < 2e-23.
//
// LDS holds TWO n x n matrices, M and P (row length n | 1, so that a column walk of doubles touches 32 distinct bank pairs).
// A product is accumulated in registers: the 256 threads form a 16 x 16 grid, thread (ty, tx) owns the elements
// (ty + 16 u, tx + 16 v) of the result, u, v < ceil(n / 16).  Between "everybody has read P" and "everybody has written P"
// stands one barrier, so no third matrix is needed.  Inner products are plain FMAs fed from LDS (per k: TILE broadcast reads
// of M, TILE contiguous reads of P, TILE^2 FMAs); no MFMA.
//
// cyb_norm1_batched_*: max_j sum_i |a_ij| of every listed matrix in one launch -- the norm table of the blocks that are too
// large for the kernel above, which the host reads once to choose their s.
#include "flat_items.h"

#include <algorithm>

namespace {

constexpr int NT = 256;
constexpr int GRID = 16; // threads per side of the thread grid

template <class T> struct Num;
template <> struct Num<double> {
    static constexpr int kMaxN = CYB_EXPM_SMALL_MAX_N_F64;
    static __device__ inline double zero() { return 0.0; }
    static __device__ inline double real(double x) { return x; }
    static __device__ inline double mul(double a, double b) { return a * b; }
    static __device__ inline double fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
    static __device__ inline double scale(double a, double s) { return a * s; }
    static __device__ inline double abs(double a) { return __builtin_fabs(a); }
    static __device__ inline double ldexp(double a, int e) { return ::ldexp(a, e); }
};
template <> struct Num<d2> {
    static constexpr int kMaxN = CYB_EXPM_SMALL_MAX_N_C128;
    static __device__ inline d2 zero() { return d2{0.0, 0.0}; }
    static __device__ inline d2 real(double x) { return d2{x, 0.0}; }
    static __device__ inline d2 mul(d2 a, d2 b) { return d2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
    static __device__ inline d2 fma(d2 a, d2 b, d2 c)
    {
        return d2{__builtin_fma(a.x, b.x, __builtin_fma(-a.y, b.y, c.x)), __builtin_fma(a.x, b.y, __builtin_fma(a.y, b.x, c.y))};
    }
    static __device__ inline d2 scale(d2 a, double s) { return d2{a.x * s, a.y * s}; }
    static __device__ inline double abs(d2 a) { return __builtin_sqrt(a.x * a.x + a.y * a.y); }
    static __device__ inline d2 ldexp(d2 a, int e) { return d2{::ldexp(a.x, e), ::ldexp(a.y, e)}; }
};

// acc(u, v) = sum_k X(ty + 16 u, k) Y(k, tx + 16 v); rows / columns beyond n are clamped to n - 1 (computed, never stored)
template <class T, int TILE>
__device__ inline void product(const T* __restrict__ X, const T* __restrict__ Y, int n, int ld, const int (&ri)[TILE], const int (&cj)[TILE],
                               T (&acc)[TILE][TILE])
{
#pragma unroll
    for (int u = 0; u < TILE; ++u)
#pragma unroll
        for (int v = 0; v < TILE; ++v) acc[u][v] = Num<T>::zero();
    for (int k = 0; k < n; ++k) {
        T a[TILE], b[TILE];
#pragma unroll
        for (int u = 0; u < TILE; ++u) a[u] = X[ri[u] + k];
#pragma unroll
        for (int v = 0; v < TILE; ++v) b[v] = Y[k * ld + cj[v]];
#pragma unroll
        for (int u = 0; u < TILE; ++u)
#pragma unroll
            for (int v = 0; v < TILE; ++v) acc[u][v] = Num<T>::fma(a[u], b[v], acc[u][v]);
    }
}

// Horner steps k = 17 .. 1 on P = I + M / 18, then s squarings; M and P in LDS, all threads of the workgroup
template <class T, int TILE> __device__ void horner_and_square(const T* M, T* P, int n, int ld, int s)
{
    const int ty = threadIdx.x / GRID, tx = threadIdx.x % GRID;
    int ri[TILE], cj[TILE]; // row offsets (in elements) and columns of the owned elements
    bool rok[TILE], cok[TILE];
#pragma unroll
    for (int u = 0; u < TILE; ++u) {
        const int i = ty + GRID * u, j = tx + GRID * u;
        rok[u] = i < n;
        cok[u] = j < n;
        ri[u] = (i < n ? i : n - 1) * ld;
        cj[u] = j < n ? j : n - 1;
    }
    T acc[TILE][TILE];
    for (int k = 17; k >= 1; --k) {
        product<T, TILE>(M, P, n, ld, ri, cj, acc);
        __syncthreads(); // every thread has read P
        const double inv = 1.0 / (double)k;
#pragma unroll
        for (int u = 0; u < TILE; ++u)
#pragma unroll
            for (int v = 0; v < TILE; ++v)
                if (rok[u] && cok[v]) {
                    T r = Num<T>::scale(acc[u][v], inv);
                    if (ri[u] == cj[v] * ld) r += Num<T>::real(1.0);
                    P[ri[u] + cj[v]] = r;
                }
        __syncthreads();
    }
    for (int q = 0; q < s; ++q) {
        product<T, TILE>(P, P, n, ld, ri, cj, acc);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < TILE; ++u)
#pragma unroll
            for (int v = 0; v < TILE; ++v)
                if (rok[u] && cok[v]) P[ri[u] + cj[v]] = acc[u][v];
        __syncthreads();
    }
}

template <class T> __global__ void __launch_bounds__(NT) expm_small_kernel(const cyb_expm_desc* __restrict__ descs, double alpha_re, double alpha_im)
{
    extern __shared__ __attribute__((aligned(16))) double smem_raw[];
    __shared__ double colsum[Num<T>::kMaxN];
    __shared__ int s_shared;
    const cyb_expm_desc d = descs[blockIdx.x];
    const int n = (int)d.n, ld = n | 1, nn = n * n;
    T* E = reinterpret_cast<T*>(d.E);
    if (d.A == nullptr) { // the zero matrix: exp = identity
        for (int idx = threadIdx.x; idx < nn; idx += NT) {
            const int i = idx / n, j = idx - i * n;
            E[(int64_t)i * d.lde + j] = Num<T>::real(i == j ? 1.0 : 0.0);
        }
        return;
    }
    T* M = reinterpret_cast<T*>(smem_raw);
    T* P = M + n * ld;
    // M = alpha * A
    for (int idx = threadIdx.x; idx < nn; idx += NT) {
        const int i = idx / n, j = idx - i * n;
        if constexpr (sizeof(T) == sizeof(double)) {
            M[i * ld + j] = alpha_re * d.A[(int64_t)i * d.lda + j];
        } else {
            const d2 alpha{alpha_re, alpha_im};
            if (d.a_is_real) {
                M[i * ld + j] = Num<d2>::scale(alpha, d.A[(int64_t)i * d.lda + j]);
            } else {
                const double* p = d.A + 2 * ((int64_t)i * d.lda + j);
                M[i * ld + j] = Num<d2>::mul(alpha, d2{p[0], p[1]});
            }
        }
    }
    __syncthreads();
    // 1-norm: column sums (one thread per column, rows ascending), maximum by thread 0
    if ((int)threadIdx.x < n) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += Num<T>::abs(M[i * ld + threadIdx.x]);
        colsum[threadIdx.x] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double norm = 0.0;
        for (int j = 0; j < n; ++j) norm = colsum[j] > norm ? colsum[j] : norm;
        int s = 0;
        if (norm > 0.5 && norm < __builtin_huge_val()) { // (NaN and inf fail the test: their result is not finite whatever s is)
            int e;
            const double m = frexp(2.0 * norm, &e); // 2 norm = m 2^e, m in [1/2, 1): ceil(log2(2 norm)) = e, or e - 1 for a power of two
            s = m == 0.5 ? e - 1 : e;
        }
        s_shared = s;
    }
    __syncthreads();
    const int s = s_shared;
    // M <- M / 2^s (exact), P = I + M / 18 (the k = 18 step of the Horner form: its product is M times the identity)
    for (int idx = threadIdx.x; idx < nn; idx += NT) {
        const int i = idx / n, j = idx - i * n;
        const T m = Num<T>::ldexp(M[i * ld + j], -s);
        M[i * ld + j] = m;
        T p = Num<T>::scale(m, 1.0 / 18.0);
        if (i == j) p += Num<T>::real(1.0);
        P[i * ld + j] = p;
    }
    __syncthreads();
    switch ((n + GRID - 1) / GRID) {
    case 1: horner_and_square<T, 1>(M, P, n, ld, s); break;
    case 2: horner_and_square<T, 2>(M, P, n, ld, s); break;
    case 3: horner_and_square<T, 3>(M, P, n, ld, s); break;
    case 4: horner_and_square<T, 4>(M, P, n, ld, s); break;
    default:
        if constexpr (Num<T>::kMaxN > 4 * GRID) {
            if (n <= 5 * GRID)
                horner_and_square<T, 5>(M, P, n, ld, s);
            else
                horner_and_square<T, 6>(M, P, n, ld, s);
        }
        break;
    }
    for (int idx = threadIdx.x; idx < nn; idx += NT) {
        const int i = idx / n, j = idx - i * n;
        E[(int64_t)i * d.lde + j] = P[i * ld + j];
    }
}

template <class T> int expm_small(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double alpha_re, double alpha_im, const char* who)
{
    constexpr int kMax = Num<T>::kMaxN;
    static_assert(kMax <= 6 * GRID, "the thread grid covers at most 6 x 6 elements per thread");
    static_assert(2 * sizeof(T) * (size_t)kMax * (size_t)(kMax | 1) <= 150 * 1024, "M and P must fit into LDS");
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "%s: bad descriptor list", who);
    std::vector<cyb_expm_desc> hd;
    int64_t max_n = 0;
    for (int64_t i = 0; i < n; ++i) {
        const cyb_expm_desc& d = descs[i];
        CYB_REQUIRE(d.n >= 0, "%s: matrix %lld: negative extent", who, (long long)i);
        if (d.n == 0) continue;
        CYB_REQUIRE(d.n <= kMax, "%s: matrix %lld: n = %lld exceeds the limit of the in-LDS kernel (%d)", who, (long long)i, (long long)d.n, kMax);
        CYB_REQUIRE(d.E && d.lde >= d.n, "%s: matrix %lld: E is NULL or lde < n", who, (long long)i);
        CYB_REQUIRE(!d.A || d.lda >= d.n, "%s: matrix %lld: lda < n", who, (long long)i);
        hd.push_back(d);
        max_n = std::max(max_n, d.n);
    }
    if (hd.empty()) return CYB_OK;
    static bool attr_set = false;
    if (!attr_set) {
        CYB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(expm_small_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(2 * sizeof(T) * (size_t)kMax * (size_t)(kMax | 1))));
        attr_set = true;
    }
    const size_t lds = 2 * sizeof(T) * (size_t)max_n * (size_t)(max_n | 1);
    void* d_descs = nullptr;
    CYB_TRY(cyb::upload_packed(ctx, {{hd.data(), sizeof(cyb_expm_desc) * hd.size(), &d_descs}}));
    hipLaunchKernelGGL(expm_small_kernel<T>, dim3((unsigned)hd.size()), dim3(NT), lds, ctx->stream, static_cast<const cyb_expm_desc*>(d_descs),
                       alpha_re, alpha_im);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

// ---- 1-norms ---------------------------------------------------------------------------------------------------------
struct NormItem {
    int32_t mat, col0;
};

// one workgroup per (matrix, 64 columns): four row groups sum the columns, the column sums are added in a fixed order and
// their maximum joins the matrix's entry through an atomic maximum on the bit pattern (non-negative doubles order like
// integers; a maximum does not depend on the order of arrival)
template <bool CPLX>
__global__ void __launch_bounds__(NT) norm1_kernel(const cyb_expm_desc* __restrict__ descs, const NormItem* __restrict__ items,
                                                   unsigned long long* __restrict__ out)
{
    __shared__ double part[NT / 64][64];
    const NormItem it = items[blockIdx.x];
    const cyb_expm_desc d = descs[it.mat];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int64_t j = (int64_t)it.col0 + lane;
    double sum = 0.0;
    if (j < d.n) {
        if (CPLX && !d.a_is_real) {
            for (int64_t i = grp; i < d.n; i += NT / 64) {
                const double* p = d.A + 2 * (i * d.lda + j);
                sum += __builtin_sqrt(p[0] * p[0] + p[1] * p[1]);
            }
        } else {
            for (int64_t i = grp; i < d.n; i += NT / 64) sum += __builtin_fabs(d.A[i * d.lda + j]);
        }
    }
    part[grp][lane] = sum;
    __syncthreads();
    if (grp == 0) {
        double v = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double w = __shfl_down(v, off);
            v = (w > v || w != w) ? w : v;
        }
        if (lane == 0) atomicMax(out + it.mat, (unsigned long long)__double_as_longlong(v));
    }
}

template <bool CPLX> int norm1_batched(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double* result_dev, const char* who)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n >= 0 && (n == 0 || (descs && result_dev)), "%s: bad arguments", who);
    if (n == 0) return CYB_OK;
    std::vector<NormItem> items;
    for (int64_t i = 0; i < n; ++i) {
        const cyb_expm_desc& d = descs[i];
        CYB_REQUIRE(d.n >= 0 && d.n <= INT32_MAX - 64, "%s: matrix %lld: bad extent", who, (long long)i);
        if (d.n == 0 || !d.A) continue; // (an absent matrix is the zero matrix)
        CYB_REQUIRE(d.lda >= d.n, "%s: matrix %lld: lda < n", who, (long long)i);
        for (int64_t c = 0; c < d.n; c += 64) items.push_back(NormItem{(int32_t)i, (int32_t)c});
    }
    CYB_REQUIRE(n <= INT32_MAX, "%s: too many matrices", who);
    CYB_HIP(hipMemsetAsync(result_dev, 0, sizeof(double) * (size_t)n, ctx->stream));
    return cyb_flat::launch(ctx, who, norm1_kernel<CPLX>, cyb_flat::arrays(cyb_flat::arr(descs, n), items), reinterpret_cast<unsigned long long*>(result_dev));
}

} // namespace

extern "C" {

int cyb_expm_small_batched_f64(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double alpha)
{
    return expm_small<double>(ctx, descs, n, alpha, 0.0, "cyb_expm_small_batched_f64");
}

int cyb_expm_small_batched_c128(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double alpha_re, double alpha_im)
{
    return expm_small<d2>(ctx, descs, n, alpha_re, alpha_im, "cyb_expm_small_batched_c128");
}

int cyb_norm1_batched_f64(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double* result_dev)
{
    return norm1_batched<false>(ctx, descs, n, result_dev, "cyb_norm1_batched_f64");
}

int cyb_norm1_batched_c128(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double* result_dev)
{
    return norm1_batched<true>(ctx, descs, n, result_dev, "cyb_norm1_batched_c128");
}

} // extern "C"
