// Grouped partial trace: every result block of a tensor-level partial trace in ONE launch.
//
// AbelianBackend::partial_trace (src/backends/abelian.cpp:2954-3081) calls block_backend->trace_partial once per block
// on the diagonal (numpy.cpp:1166-1195: transpose, reshape, trace) and adds the results that share a destination with one
// Block::operator+ each (:3026-3029).  Here an *output* record is one result block and a *term* record one contributing
// source block, read in place through its strides (walking the SUM of the two strides of a traced pair walks the diagonal of
// that pair).  Every output element has exactly one owner which adds its terms in a fixed order: no float atomics, no
// zero fill, no second pass, bit-identical from run to run.
//
// The owner of an output element is chosen per output record on the host from R (number of output elements) and A (number
// of addends per element, summed over the terms):
//   * lane  (1 lane per element):   A < 64, or R fills the chip by itself.  Lanes are adjacent along the innermost
//     remaining axis, so a source whose innermost remaining axis is contiguous is read in full 512-byte wave accesses.
//   * wave  (64 lanes per element): the lanes stride over the traced multi-index; shuffle tree of fixed shape.
//   * group (256 lanes per element): few elements with very many addends (trace_full); the four wave sums are added by
//     lane 0 in wave order through LDS.
#include "flat_items.h"

#include <algorithm>

namespace {

constexpr int NT = 256;
constexpr int kPairs = CYB_TRACE_MAX_PAIRS;

struct Item {
    int32_t out;   // output record
    int32_t lanes; // owner of one output element: 1, 64 or 256 lanes
    int64_t start, count; // range of output elements of this workgroup
};

template <class T> __device__ inline T zero_of();
template <> __device__ inline double zero_of<double>() { return 0.0; }
template <> __device__ inline d2 zero_of<d2>() { return d2{0.0, 0.0}; }

__device__ inline double shfl_down_(double v, int o) { return __shfl_down(v, o); }
__device__ inline d2 shfl_down_(d2 v, int o) { return d2{__shfl_down(v.x, o), __shfl_down(v.y, o)}; }

// multi-index of output element `e` (C order over the remaining axes)
__device__ inline void decode(const cyb_trace_out& o, int64_t e, int64_t (&idx)[CYB_MAX_NDIM])
{
#pragma unroll
    for (int k = CYB_MAX_NDIM - 1; k >= 0; --k) {
        idx[k] = 0;
        if (k < o.ndim) {
            const int64_t q = e / o.shape[k];
            idx[k] = e - q * o.shape[k];
            e = q;
        }
    }
}

__device__ inline int64_t base_of(const GLOBAL_AS cyb_trace_term* tm, int ndim, const int64_t (&idx)[CYB_MAX_NDIM])
{
    int64_t b = 0;
#pragma unroll
    for (int k = 0; k < CYB_MAX_NDIM; ++k)
        if (k < ndim) b += idx[k] * tm->rem_strides[k];
    return b;
}

template <class T>
__global__ void __launch_bounds__(NT) trace_grouped_kernel(const cyb_trace_out* __restrict__ outs, const cyb_trace_term* __restrict__ terms,
                                                           const Item* __restrict__ items)
{
    __shared__ T red[NT / 64];
    const Item it = items[blockIdx.x];
    const cyb_trace_out o = outs[it.out];
    GLOBAL_AS T* dst = (GLOBAL_AS T*)o.dst;
    const int64_t end = it.start + it.count;
    int64_t idx[CYB_MAX_NDIM];

    if (it.lanes == 1) {
        for (int64_t e = it.start + threadIdx.x; e < end; e += NT) {
            decode(o, e, idx);
            T acc = zero_of<T>();
            for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t) {
                const GLOBAL_AS cyb_trace_term* tm = (const GLOBAL_AS cyb_trace_term*)(terms + t);
                const GLOBAL_AS T* src = (const GLOBAL_AS T*)tm->src + base_of(tm, o.ndim, idx);
                // unused pairs have extent 1 and stride 0 (set by the entry point)
                const int64_t n0 = tm->pair_extent[0], n1 = tm->pair_extent[1], n2 = tm->pair_extent[2], n3 = tm->pair_extent[3];
                const int64_t s0 = tm->pair_stride[0], s1 = tm->pair_stride[1], s2 = tm->pair_stride[2], s3 = tm->pair_stride[3];
                for (int64_t i3 = 0; i3 < n3; ++i3)
                    for (int64_t i2 = 0; i2 < n2; ++i2)
                        for (int64_t i1 = 0; i1 < n1; ++i1) {
                            const GLOBAL_AS T* p = src + i3 * s3 + i2 * s2 + i1 * s1;
                            for (int64_t i0 = 0; i0 < n0; ++i0) acc += p[i0 * s0];
                        }
            }
            dst[e] = acc;
        }
        return;
    }

    // 64 or 256 lanes per output element: the lanes stride over the traced multi-index of every term
    const int lanes = it.lanes;
    const int lane = threadIdx.x & (lanes - 1);
    const int per_round = NT / lanes;
    for (int64_t e0 = it.start; e0 < end; e0 += per_round) {
        const int64_t e = e0 + threadIdx.x / lanes; // (uniform in a wave)
        T acc = zero_of<T>();
        if (e < end) {
            decode(o, e, idx);
            for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t) {
                const GLOBAL_AS cyb_trace_term* tm = (const GLOBAL_AS cyb_trace_term*)(terms + t);
                const GLOBAL_AS T* src = (const GLOBAL_AS T*)tm->src + base_of(tm, o.ndim, idx);
                const int64_t n0 = tm->pair_extent[0], n1 = tm->pair_extent[1], n2 = tm->pair_extent[2], n3 = tm->pair_extent[3];
                const int64_t s0 = tm->pair_stride[0], s1 = tm->pair_stride[1], s2 = tm->pair_stride[2], s3 = tm->pair_stride[3];
                const int64_t tot = n0 * n1 * n2 * n3;
                if (tm->n_pairs <= 1) {
                    for (int64_t j = lane; j < tot; j += lanes) acc += src[j * s0];
                } else {
                    for (int64_t j = lane; j < tot; j += lanes) {
                        int64_t r = j;
                        const int64_t i0 = r % n0;
                        r /= n0;
                        const int64_t i1 = r % n1;
                        r /= n1;
                        const int64_t i2 = r % n2;
                        const int64_t i3 = r / n2;
                        acc += src[i0 * s0 + i1 * s1 + i2 * s2 + i3 * s3];
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += shfl_down_(acc, off);
        if (lanes == 64) {
            if (lane == 0 && e < end) dst[e] = acc;
        } else {
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
            __syncthreads();
            if (threadIdx.x == 0) dst[e] = ((red[0] + red[1]) + red[2]) + red[3];
            __syncthreads();
        }
    }
}

template <class T>
int trace_grouped(cyb_ctx_t ctx, const cyb_trace_out* outs, int64_t n_outs, const cyb_trace_term* terms, int64_t n_terms, const char* who)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n_outs >= 0 && n_terms >= 0 && (n_outs == 0 || outs) && (n_terms == 0 || terms), "%s: bad lists", who);
    if (n_outs == 0) return CYB_OK;
    std::vector<cyb_trace_term> ht(terms, terms + n_terms);
    std::vector<int64_t> addends((size_t)n_terms, 0);
    for (int64_t t = 0; t < n_terms; ++t) {
        cyb_trace_term& tm = ht[(size_t)t];
        CYB_REQUIRE(tm.n_pairs >= 0 && tm.n_pairs <= kPairs, "%s: term %lld: %d traced pairs (at most %d)", who, (long long)t, tm.n_pairs, kPairs);
        int64_t a = 1;
        for (int p = 0; p < kPairs; ++p) {
            if (p >= tm.n_pairs) tm.pair_extent[p] = 1, tm.pair_stride[p] = 0;
            CYB_REQUIRE(tm.pair_extent[p] >= 0, "%s: term %lld: negative extent", who, (long long)t);
            a *= tm.pair_extent[p];
        }
        addends[(size_t)t] = a;
    }
    // owner per output record, work items per workgroup
    struct Plan {
        int lanes;
        int64_t total;
    };
    std::vector<Plan> plan((size_t)n_outs);
    int64_t lane_total = 0;
    for (int64_t i = 0; i < n_outs; ++i) {
        const cyb_trace_out& o = outs[i];
        CYB_REQUIRE(o.ndim >= 0 && o.ndim <= CYB_MAX_NDIM, "%s: output %lld: ndim %d out of range", who, (long long)i, o.ndim);
        CYB_REQUIRE(o.first_term >= 0 && o.n_terms >= 0 && o.first_term + o.n_terms <= n_terms,
                    "%s: output %lld: bad term range [%lld, +%lld)", who, (long long)i, (long long)o.first_term, (long long)o.n_terms);
        int64_t R = 1;
        for (int k = 0; k < o.ndim; ++k) {
            CYB_REQUIRE(o.shape[k] >= 0, "%s: output %lld: negative extent", who, (long long)i);
            R *= o.shape[k];
        }
        CYB_REQUIRE(R == 0 || o.dst, "%s: output %lld: dst is NULL", who, (long long)i);
        int64_t A = 0;
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t) {
            CYB_REQUIRE(o.ndim + 2 * ht[(size_t)t].n_pairs <= CYB_MAX_NDIM, "%s: term %lld: more than %d source axes", who, (long long)t, CYB_MAX_NDIM);
            CYB_REQUIRE(R == 0 || addends[(size_t)t] == 0 || ht[(size_t)t].src, "%s: term %lld: src is NULL", who, (long long)t);
            A += addends[(size_t)t];
        }
        // 65536 lanes = one 256-thread workgroup on each of the 256 CUs; 1024 waves = one per SIMD
        int lanes = 1;
        if (A >= 64 && R < 65536) lanes = (A < 4096 || R >= 1024) ? 64 : 256;
        plan[(size_t)i] = Plan{lanes, R};
        if (lanes == 1) lane_total += R;
    }
    // lane regime: about 2048 workgroups for the launch, at least 4 and at most 256 elements per lane
    int64_t chunk = (lane_total / 2048 + 1023) & ~(int64_t)1023;
    chunk = std::min<int64_t>(std::max<int64_t>(chunk, 4 * NT), 256 * NT);
    std::vector<Item> items;
    for (int64_t i = 0; i < n_outs; ++i) {
        const Plan& p = plan[(size_t)i];
        const int64_t step = p.lanes == 1 ? chunk : NT / p.lanes; // wave: 4 elements (one per wave), group: 1 element per workgroup
        for (int64_t s = 0; s < p.total; s += step) items.push_back(Item{(int32_t)i, p.lanes, s, std::min(step, p.total - s)});
    }
    return cyb_flat::launch(ctx, who, trace_grouped_kernel<T>, cyb_flat::arrays(cyb_flat::arr(outs, n_outs), ht, items));
}

} // namespace

extern "C" {

int cyb_trace_grouped_f64(cyb_ctx_t ctx, const cyb_trace_out* outs, int64_t n_outs, const cyb_trace_term* terms, int64_t n_terms)
{
    return trace_grouped<double>(ctx, outs, n_outs, terms, n_terms, "cyb_trace_grouped_f64");
}

int cyb_trace_grouped_c128(cyb_ctx_t ctx, const cyb_trace_out* outs, int64_t n_outs, const cyb_trace_term* terms, int64_t n_terms)
{
    return trace_grouped<d2>(ctx, outs, n_outs, terms, n_terms, "cyb_trace_grouped_c128");
}

} // extern "C"
