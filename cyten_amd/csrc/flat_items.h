// One workgroup per work item over a flat range: the machinery shared by the memory-bound kernels that give a WORKGROUP the
// elements [start, start + count) of one record (blockops.hip, krylov_vec.hip, tree_axis.hip, place_plan.hip and the copy
// bodies of copy_kernels.h), the launch tail of every kernel that reads its records and items from one packed upload, and the
// fixed-order reduction behind the promise "no float atomics, fixed summation order, bit-identical from run to run".
//   * host: every record of totals[i] elements is cut into items of at most `chunk` elements (cut); the chunk comes from the
//     size of the whole list by one of the named rules below.  A different cut is a different summation order, so a rule
//     returns for every total what it has always returned (tests/flat_items_cut.cpp holds literals).
//   * launch: the arrays of a launch travel in ONE packed upload, the grid is one workgroup per K items (launch).
//     wave_items.h's launch_items is the K = 4 use.
//   * reduction: a lane accumulates as its kernel sees fit; from there the order is fixed here and nowhere else: the xor
//     butterfly over the wave (wave_reduce), the four wave results in wave order by thread 0 (block_reduce), one partial per
//     item, the partials strided over the 256 threads of ONE workgroup per result and reduced the same way (stage2_kernel).
//     two_stage is the host chain of both stages.
// The item, the rules and the cutter compile without HIP, so that a plain C++ program can check them
// (tests/flat_items_cut.cpp).
#pragma once
#ifdef __HIPCC__
#include "common.h"
#endif

#include <algorithm>
#include <cstdint>
#include <tuple>
#include <utility>
#include <vector>

namespace cyb_flat {

constexpr int NT = 256, WAVE = 64, WAVES = NT / WAVE;

// elements [start, start + count) of record `desc`
struct Item {
    int32_t desc;
    int32_t pad;
    int64_t start, count;
};

// ---- host: chunk rules and the cutter ----------------------------------------------------------------------------------

// about 2048 work items for a list of `total` elements, lo <= chunk <= hi, a multiple of `step` (a power of two)
inline int64_t chunk_rule(int64_t total, int64_t lo, int64_t hi, int64_t step)
{
    const int64_t c = ((total / 2048) + step - 1) & ~(step - 1);
    return std::min(hi, std::max(lo, c));
}

constexpr int64_t kMaxChunk = 1 << 16; // largest number of 8-byte elements per work item
// 8-byte elements: 64 K once the list fills the chip eight workgroups per CU deep, smaller (down to 8 K, always a multiple
// of 1024) for the 10-100 MB lists of one tensor operation, which would otherwise run as a few hundred workgroups on 256 CUs
inline int64_t chunk_real(int64_t total) { return chunk_rule(total, 8192, kMaxChunk, 1024); }
// complex elements read by both operands of an inner product: 32 K (512 KB of each operand) down to 4 K, a multiple of 512.
// NOT chunk_real(2 * total) / 2 at every total
inline int64_t chunk_complex(int64_t total) { return chunk_rule(total, 4096, 1 << 15, 512); }

// Appends the items of record i = 0, 1, ... (totals[i] elements, none for an empty record), each of at most `chunk` elements,
// in ascending order.  false, and nothing appended: the list would hold 2^31 items or more (a grid is 32 bits wide)
inline bool cut(std::vector<Item>& items, const std::vector<int64_t>& totals, int64_t chunk)
{
    uint64_t n = items.size();
    for (int64_t t : totals) n += t > 0 ? (uint64_t)((t - 1) / chunk + 1) : 0;
    if (n >= ((uint64_t)1 << 31)) return false;
    items.reserve((size_t)n);
    for (size_t i = 0; i < totals.size(); ++i)
        for (int64_t s = 0; s < totals[i]; s += chunk) items.push_back(Item{(int32_t)i, 0, s, std::min(chunk, totals[i] - s)});
    return true;
}

inline int64_t sum_of(const std::vector<int64_t>& totals)
{
    int64_t grand = 0;
    for (int64_t t : totals) grand += t;
    return grand;
}

#ifdef __HIPCC__
#define CYB_CUT(who, items, totals, chunk) CYB_REQUIRE(cyb_flat::cut(items, totals, chunk), "%s: too many work items", who)

// ---- host: the launch tail ---------------------------------------------------------------------------------------------

// a host array that travels to the device with a launch
template <class T> struct Arr {
    const T* p;
    size_t n;
};
template <class T> inline Arr<T> arr(const std::vector<T>& v) { return Arr<T>{v.data(), v.size()}; }
template <class T> inline Arr<T> arr(const T* p, int64_t n) { return Arr<T>{p, (size_t)n}; }
template <class T> inline Arr<T> arr(const Arr<T>& a) { return a; }
template <class... V> inline auto arrays(const V&... v) { return std::make_tuple(arr(v)...); }

template <int K, class... A, class F, size_t... Is>
int with_arrays_(cyb_ctx_t ctx, const char* who, size_t n_items, const std::tuple<Arr<A>...>& a, F&& enqueue, std::index_sequence<Is...>)
{
    CYB_REQUIRE(n_items < ((size_t)1 << 31), "%s: too many work items", who);
    void* dev[sizeof...(A)] = {};
    // An empty array beside items travels as 8 bytes nobody reads, borrowed from the first array (the records, which exist
    // when items do): the term list of outputs without terms.  Without items nothing is borrowed: an empty array is 0 bytes
    // and its device address nullptr (the reductions of an empty list, which upload their segment table alone).
    const auto& first = std::get<0>(a);
    static_assert(sizeof(*first.p) >= 8, "the first array lends 8 bytes");
    const size_t lent = n_items && first.n ? 8 : 0;
    CYB_TRY(cyb::upload_packed(ctx, {{std::get<Is>(a).n ? (const void*)std::get<Is>(a).p : (const void*)first.p,
                                      std::get<Is>(a).n ? sizeof(A) * std::get<Is>(a).n : lent, &dev[Is]}...}));
    CYB_TRY(enqueue(dim3((unsigned)((n_items + K - 1) / K)), static_cast<const A*>(dev[Is])...));
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

// Uploads `arrays` in one packed upload and calls enqueue(grid, device address of every array...) -> int, which enqueues what
// reads them; grid = one workgroup per K of the n_items items.
template <int K = 1, class... A, class F>
int with_arrays(cyb_ctx_t ctx, const char* who, size_t n_items, const std::tuple<Arr<A>...>& arrays, F&& enqueue)
{
    return with_arrays_<K>(ctx, who, n_items, arrays, enqueue, std::index_sequence_for<A...>{});
}

// kernel<<<one workgroup per K items, NT>>>(arrays..., extra...); the items are the last array.  Nothing happens without items.
template <int K = 1, class... P, class... A, class... X>
int launch(cyb_ctx_t ctx, const char* who, void (*kernel)(P...), const std::tuple<Arr<A>...>& arrays, X... extra)
{
    const size_t n_items = std::get<sizeof...(A) - 1>(arrays).n;
    if (n_items == 0) return CYB_OK;
    return with_arrays<K>(ctx, who, n_items, arrays, [&](dim3 grid, const A*... dev) {
        hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, ctx->stream, dev..., extra...);
        return CYB_OK;
    });
}

// ---- device: the fixed-order reduction ---------------------------------------------------------------------------------

// item blockIdx.x of ONE record of n elements whose descriptor and chunk travel as kernel arguments (no upload)
__device__ __forceinline__ Item nth_item(int64_t chunk, int64_t n)
{
    const int64_t start = (int64_t)blockIdx.x * chunk;
    return Item{0, 0, start, min(chunk, n - start)};
}

// the combining operations: both start from 0.0
struct Sum {
    __device__ static __forceinline__ double op(double a, double b) { return a + b; }
};
// max that keeps a NaN of either side (fmax would return the other operand): np.max(np.abs(x)) is NaN when x holds one
struct NanMax {
    __device__ static __forceinline__ double op(double a, double b) { return (a > b || a != a) ? a : b; }
};

template <class Op> __device__ __forceinline__ double wave_reduce(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::op(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) { return wave_reduce<Sum>(v); }

// The workgroup's reduction of `acc` (C numbers per thread): every wave by wave_reduce, then thread 0 combines the four wave
// results in wave order.  Valid in thread 0 only.  `red` is the CALLER's LDS, double[C][WAVES]: the step holds one barrier,
// after the writes, so a second call with the same `red` may overwrite it while thread 0 still reads the first result -- give
// a second call its own array or put a __syncthreads() between the two.
template <int C, class Op = Sum> __device__ __forceinline__ void block_reduce(double (&acc)[C], double (*red)[WAVES])
{
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = wave_reduce<Op>(acc[c]);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) red[c][threadIdx.x / WAVE] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double r = red[c][0];
            for (int q = 1; q < WAVES; ++q) r = Op::op(r, red[c][q]);
            acc[c] = r;
        }
    }
}

// acc[c] = Op over table[(e * stride + col) * C + c], e in [e0, e1) strided over the workgroup; valid in thread 0
template <int C, class Op>
__device__ __forceinline__ void reduce_rows(double (&acc)[C], const double* __restrict__ table, int64_t e0, int64_t e1, int64_t stride, int64_t col,
                                            double (*red)[WAVES])
{
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += NT) {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = Op::op(acc[c], table[(e * stride + col) * C + c]);
    }
    block_reduce<C, Op>(acc, red);
}

// result[C * g + c] = Op over partial[C * e + c], e in seg[g] .. seg[g + 1] (one workgroup per result g, fixed order);
// seg == nullptr: the single range [0, n)
template <int C, class Op>
__global__ void __launch_bounds__(NT) stage2_kernel(const double* __restrict__ partial, const int64_t* __restrict__ seg, int64_t n,
                                                    double* __restrict__ result)
{
    __shared__ double red[C][WAVES];
    double acc[C];
    reduce_rows<C, Op>(acc, partial, seg ? seg[blockIdx.x] : 0, seg ? seg[blockIdx.x + 1] : n, 1, 0, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) result[C * (int64_t)blockIdx.x + c] = acc[c];
    }
}

// The host chain of a two-stage reduction: C partials per item in workspace slot 0, stage1(partial) -> int enqueues the
// kernel that writes partial[C * item + c] (not called without items), then one workgroup per group reduces them into
// result_dev[C * group + c].  d_seg: device table of n_groups + 1 item bounds, or nullptr for ONE group over all items.
// An empty list still writes its zero results.
template <int C, class Op, class F>
int two_stage(cyb_ctx_t ctx, size_t n_items, const int64_t* d_seg, int64_t n_groups, double* result_dev, F&& stage1)
{
    void* ws = nullptr;
    CYB_TRY(ctx->workspace(sizeof(double) * C * std::max<size_t>(n_items, 1), &ws));
    if (n_items) CYB_TRY(stage1(static_cast<double*>(ws)));
    hipLaunchKernelGGL((stage2_kernel<C, Op>), dim3((unsigned)n_groups), dim3(NT), 0, ctx->stream, static_cast<const double*>(ws), d_seg,
                       (int64_t)n_items, result_dev);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}
#endif // __HIPCC__

} // namespace cyb_flat
