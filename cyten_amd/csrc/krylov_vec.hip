// Vector kernels of the Krylov solvers on complex vectors (gfx950).
//
// cyb_dot_batched_c128: the inner product sum_i conj(x_i) y_i of a list of interleaved complex vectors -- the
// `inner` of the complex Krylov recurrences (Lanczos / Arnoldi on complex128 pools, krylov_based.cpp:563-589,
// 855-870) and of HipBlockBackend.inner_many on complex block lists (abelian.cpp:2159-2211).  One pass over both
// operands with 16-byte accesses; the same deterministic two-stage reduction as the float64 reductions of
// blockops.hip (fixed work items per list, fixed summation order, no float atomics): bit-identical from run to run.
#include "common.h"

#include <algorithm>

namespace {

#define GLOBAL_AS __attribute__((address_space(1)))
typedef double d2v __attribute__((ext_vector_type(2)));

constexpr int NT = 256;
constexpr int64_t CHUNK = 1 << 15; // largest number of complex elements per work item (512 KB of each operand)

// Work-item size for a list of `total` complex elements: 32 K once the list fills the chip eight workgroups per CU deep,
// smaller (down to 4 K, a multiple of 512) for the 10-100 MB vectors of one Krylov step
static int64_t chunk_for(int64_t total)
{
    int64_t c = ((total / 2048) + 511) & ~(int64_t)511;
    return std::min(CHUNK, std::max<int64_t>(4096, c));
}

struct Item {
    int32_t desc;
    int32_t pad;
    int64_t start, count;
};

struct CVecDev {
    const double* x;
    const double* y;
    int64_t n;
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// partial[2 * blockIdx.x + {0, 1}] = (re, im) of sum over the item of conj(x) y
__device__ __forceinline__ void cdot_stage1_body(const CVecDev& d, const Item& it, double* __restrict__ partial)
{
    __shared__ double red[2][NT / 64];
    const GLOBAL_AS d2v* x = (const GLOBAL_AS d2v*)d.x + it.start;
    const GLOBAL_AS d2v* y = (const GLOBAL_AS d2v*)d.y + it.start;
    // two independent accumulator pairs: two 16-byte loads of each operand in flight per lane
    double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
    int64_t i = threadIdx.x;
    for (; i + NT < it.count; i += 2 * NT) {
        const d2v a = x[i], b = y[i], a1 = x[i + NT], b1 = y[i + NT];
        re0 += a.x * b.x + a.y * b.y;
        im0 += a.x * b.y - a.y * b.x;
        re1 += a1.x * b1.x + a1.y * b1.y;
        im1 += a1.x * b1.y - a1.y * b1.x;
    }
    if (i < it.count) {
        const d2v a = x[i], b = y[i];
        re0 += a.x * b.x + a.y * b.y;
        im0 += a.x * b.y - a.y * b.x;
    }
    const double re = wave_sum(re0 + re1), im = wave_sum(im0 + im1);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = re;
        red[1][threadIdx.x >> 6] = im;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0][0], s = red[1][0];
        for (int q = 1; q < NT / 64; ++q) {
            r += red[0][q];
            s += red[1][q];
        }
        partial[2 * blockIdx.x] = r;
        partial[2 * blockIdx.x + 1] = s;
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
    const int64_t start = (int64_t)blockIdx.x * chunk;
    const Item it{0, 0, start, min(chunk, d.n - start)};
    cdot_stage1_body(d, it, partial);
}

// result[0..1] = sum over the n_items partial pairs, in a fixed order (one workgroup)
__global__ void __launch_bounds__(NT) cdot_stage2_kernel(const double* __restrict__ partial, int64_t n_items, double* __restrict__ result)
{
    __shared__ double red[2][NT / 64];
    double re = 0.0, im = 0.0;
    for (int64_t e = threadIdx.x; e < n_items; e += NT) {
        re += partial[2 * e];
        im += partial[2 * e + 1];
    }
    re = wave_sum(re);
    im = wave_sum(im);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = re;
        red[1][threadIdx.x >> 6] = im;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0][0], s = red[1][0];
        for (int q = 1; q < NT / 64; ++q) {
            r += red[0][q];
            s += red[1][q];
        }
        result[0] = r;
        result[1] = s;
    }
}

} // namespace

extern "C" {

int cyb_dot_batched_c128(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev)
{
    CYB_REQUIRE(ctx && result_dev, "cyb_dot_batched_c128: NULL argument");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "cyb_dot_batched_c128: bad descriptor list");
    std::vector<CVecDev> hv((size_t)n);
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        CYB_REQUIRE(descs[i].n >= 0, "cyb_dot_batched_c128: desc %lld: negative length", (long long)i);
        CYB_REQUIRE(descs[i].n == 0 || (descs[i].x && descs[i].y), "cyb_dot_batched_c128: desc %lld: NULL operand", (long long)i);
        hv[(size_t)i] = CVecDev{descs[i].x, descs[i].y, descs[i].n};
        total += descs[i].n;
    }
    const int64_t chunk = chunk_for(total);
    if (n == 1 && total > 0) { // ONE vector: no descriptor upload
        const int64_t n_items = cdiv64(total, chunk);
        void* ws = nullptr;
        CYB_TRY(ctx->workspace(2 * sizeof(double) * (size_t)n_items, &ws));
        hipLaunchKernelGGL(cdot_stage1_one_kernel, dim3((unsigned)n_items), dim3(NT), 0, ctx->stream, hv[0], chunk, static_cast<double*>(ws));
        hipLaunchKernelGGL(cdot_stage2_kernel, dim3(1), dim3(NT), 0, ctx->stream, static_cast<const double*>(ws), n_items, result_dev);
        CYB_HIP(hipGetLastError());
        return CYB_OK;
    }
    std::vector<Item> items;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t s = 0; s < descs[i].n; s += chunk) items.push_back(Item{(int32_t)i, 0, s, std::min(chunk, descs[i].n - s)});
    void* ws = nullptr;
    CYB_TRY(ctx->workspace(2 * sizeof(double) * std::max<size_t>(items.size(), 1), &ws));
    if (!items.empty()) {
        void *d_descs = nullptr, *d_items = nullptr;
        CYB_TRY(cyb::upload_packed(ctx, {{hv.data(), sizeof(CVecDev) * hv.size(), &d_descs}, {items.data(), sizeof(Item) * items.size(), &d_items}}));
        hipLaunchKernelGGL(cdot_stage1_kernel, dim3((unsigned)items.size()), dim3(NT), 0, ctx->stream,
                           static_cast<const CVecDev*>(d_descs), static_cast<const Item*>(d_items), static_cast<double*>(ws));
    }
    // (an empty list still writes its zero result)
    hipLaunchKernelGGL(cdot_stage2_kernel, dim3(1), dim3(NT), 0, ctx->stream, static_cast<const double*>(ws), (int64_t)items.size(), result_dev);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

} // extern "C"
