// Weighted partial trace into strided tiles: every result block of a fusion-tree partial trace in ONE launch.
//
// FusionTreeBackend::partial_trace, step 2 (src/backends/fusion_tree_backend.cpp:3092-3159), makes per pair of tree blocks
// get_item, reshape, trace_partial, reshape, mul by the B-symbol factor (:3149), get_item of the destination tile, operator+
// and set_item.  Here an *output* record is one destination tile -- a strided N-d view into a coupled block -- and a *term*
// record one contributing old tree pair with its coefficient, read in place through its strides (walking the SUM of the two
// strides of a traced pair walks the diagonal of that pair):
//   out[r] = sum_t c_t * (sum_tau src_t[r . rem_strides_t + tau . pair_stride_t])
// Every output element has exactly one owner which adds its terms in a fixed order and multiplies each term's sum by its
// coefficient once: no float atomics, no zero fill, no second pass, bit-identical from run to run; an output with no terms
// is written as zeros.
//
// The owner of an output element is chosen per output record on the host from R (number of output elements) and A (number
// of addends per element, summed over the terms), with the thresholds of trace_grouped.hip:
//   * lane  (1 lane per element):   A < 64, or R fills the chip by itself (two-site tensors: tiny traced extents, many
//     small terms, many elements).  Lanes are adjacent along the innermost remaining axis.  A float64 record whose
//     innermost remaining axis is contiguous in the destination and in every source, with an even extent and with every
//     other stride and every base address a multiple of 16 bytes, is run on pairs of elements: 16-byte loads and stores.
//     (A complex128 element is a 16-byte access as it stands.)
//   * wave  (64 lanes per element): the lanes stride over the traced multi-index of one term; shuffle tree of fixed
//     shape per term, lane 0 multiplies by the coefficient and adds.
//   * group (256 lanes per element): few elements with very many addends (a bond-pair trace, the full trace); the four
//     wave sums of a term are added by lane 0 in wave order through LDS.
#include "flat_items.h"

#include <algorithm>

namespace {

constexpr int NT = 256;
constexpr int kPairs = CYB_TRACE_MAX_PAIRS;
typedef cyb_trace_weighted_out Out;
typedef cyb_trace_weighted_term Term;

// what a lane holds per output element: one double, two adjacent doubles, or one complex number
enum { kF64 = 0, kF64x2 = 1, kC128 = 2 };
template <int MODE> struct Acc { typedef d2 type; };
template <> struct Acc<kF64> { typedef double type; };

struct Item {
    int32_t out;   // output record
    int16_t lanes; // owner of one output element: 1, 64 or 256 lanes
    int16_t mode;
    int64_t start, count; // range of output elements (kF64x2: of element pairs) of this workgroup
};

template <class T> __device__ inline T zero_of();
template <> __device__ inline double zero_of<double>() { return 0.0; }
template <> __device__ inline d2 zero_of<d2>() { return d2{0.0, 0.0}; }

__device__ inline double shfl_down_(double v, int o) { return __shfl_down(v, o); }
__device__ inline d2 shfl_down_(d2 v, int o) { return d2{__shfl_down(v.x, o), __shfl_down(v.y, o)}; }

// `off` counts elements of the record's type (kF64x2: doubles); a float64 source under the c128 entry counts doubles
template <int MODE> __device__ inline typename Acc<MODE>::type load_(const GLOBAL_AS double* src, int64_t off, bool real)
{
    if constexpr (MODE == kF64) {
        return src[off];
    } else if constexpr (MODE == kF64x2) {
        return *(const GLOBAL_AS d2*)(src + off);
    } else {
        if (real) return d2{src[off], 0.0};
        return *(const GLOBAL_AS d2*)(src + 2 * off);
    }
}

template <int MODE> __device__ inline void store_(GLOBAL_AS double* dst, int64_t off, typename Acc<MODE>::type v)
{
    if constexpr (MODE == kF64) {
        dst[off] = v;
    } else if constexpr (MODE == kF64x2) {
        *(GLOBAL_AS d2*)(dst + off) = v;
    } else {
        *(GLOBAL_AS d2*)(dst + 2 * off) = v;
    }
}

// acc += c * s, once per term and output element
template <int MODE> __device__ inline void add_scaled(typename Acc<MODE>::type& acc, double cr, double ci, typename Acc<MODE>::type s)
{
    if constexpr (MODE == kC128) {
        acc.x += cr * s.x - ci * s.y;
        acc.y += cr * s.y + ci * s.x;
    } else {
        acc += cr * s;
    }
}

// multi-index of output element `e` (C order over the remaining axes; kF64x2: the innermost index counts doubles)
template <int MODE> __device__ inline void decode(const Out& o, int64_t e, int64_t (&idx)[CYB_MAX_NDIM])
{
#pragma unroll
    for (int k = CYB_MAX_NDIM - 1; k >= 0; --k) {
        idx[k] = 0;
        if (k < o.ndim) {
            const int64_t q = e / o.shape[k];
            idx[k] = e - q * o.shape[k];
            if (MODE == kF64x2 && k == o.ndim - 1) idx[k] *= 2;
            e = q;
        }
    }
}

__device__ inline int64_t dot_(const GLOBAL_AS int64_t* strides, int ndim, const int64_t (&idx)[CYB_MAX_NDIM])
{
    int64_t b = 0;
#pragma unroll
    for (int k = 0; k < CYB_MAX_NDIM; ++k)
        if (k < ndim) b += idx[k] * strides[k];
    return b;
}

template <int MODE> __device__ inline void lane_regime(const Out& o, const GLOBAL_AS Out* og, const Term* __restrict__ terms, const Item& it)
{
    typedef typename Acc<MODE>::type T;
    GLOBAL_AS double* dst = (GLOBAL_AS double*)o.dst;
    const int64_t end = it.start + it.count;
    int64_t idx[CYB_MAX_NDIM];
    for (int64_t e = it.start + threadIdx.x; e < end; e += NT) {
        decode<MODE>(o, e, idx);
        T acc = zero_of<T>();
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t) {
            const GLOBAL_AS Term* tm = (const GLOBAL_AS Term*)(terms + t);
            const GLOBAL_AS double* src = (const GLOBAL_AS double*)tm->src;
            const bool real = tm->src_real != 0;
            const int64_t base = dot_(tm->rem_strides, o.ndim, idx);
            // unused pairs have extent 1 and stride 0 (set by the entry point)
            const int64_t n0 = tm->pair_extent[0], n1 = tm->pair_extent[1], n2 = tm->pair_extent[2], n3 = tm->pair_extent[3];
            const int64_t s0 = tm->pair_stride[0], s1 = tm->pair_stride[1], s2 = tm->pair_stride[2], s3 = tm->pair_stride[3];
            T s = zero_of<T>();
            for (int64_t i3 = 0; i3 < n3; ++i3)
                for (int64_t i2 = 0; i2 < n2; ++i2)
                    for (int64_t i1 = 0; i1 < n1; ++i1) {
                        const int64_t p = base + i3 * s3 + i2 * s2 + i1 * s1;
                        for (int64_t i0 = 0; i0 < n0; ++i0) s += load_<MODE>(src, p + i0 * s0, real);
                    }
            add_scaled<MODE>(acc, tm->coeff_re, tm->coeff_im, s);
        }
        store_<MODE>(dst, dot_(og->dst_strides, o.ndim, idx), acc);
    }
}

// 64 or 256 lanes per output element: the lanes stride over the traced multi-index of one term at a time
template <int MODE>
__device__ inline void wide_regime(const Out& o, const GLOBAL_AS Out* og, const Term* __restrict__ terms, const Item& it,
                                   typename Acc<MODE>::type* red)
{
    typedef typename Acc<MODE>::type T;
    GLOBAL_AS double* dst = (GLOBAL_AS double*)o.dst;
    const int64_t end = it.start + it.count;
    int64_t idx[CYB_MAX_NDIM];
    const int lanes = it.lanes;
    const int lane = threadIdx.x & (lanes - 1);
    const int per_round = NT / lanes;
    for (int64_t e0 = it.start; e0 < end; e0 += per_round) {
        const int64_t e = e0 + threadIdx.x / lanes; // (uniform in a wave; lanes == 256: in the workgroup, and e < end)
        const bool active = e < end;
        if (active) decode<MODE>(o, e, idx);
        T acc = zero_of<T>();
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t) {
            const GLOBAL_AS Term* tm = (const GLOBAL_AS Term*)(terms + t);
            T s = zero_of<T>();
            if (active) {
                const GLOBAL_AS double* src = (const GLOBAL_AS double*)tm->src;
                const bool real = tm->src_real != 0;
                const int64_t base = dot_(tm->rem_strides, o.ndim, idx);
                const int64_t n0 = tm->pair_extent[0], n1 = tm->pair_extent[1], n2 = tm->pair_extent[2], n3 = tm->pair_extent[3];
                const int64_t s0 = tm->pair_stride[0], s1 = tm->pair_stride[1], s2 = tm->pair_stride[2], s3 = tm->pair_stride[3];
                const int64_t tot = n0 * n1 * n2 * n3;
                if (tm->n_pairs <= 1) {
                    for (int64_t j = lane; j < tot; j += lanes) s += load_<MODE>(src, base + j * s0, real);
                } else {
                    for (int64_t j = lane; j < tot; j += lanes) {
                        int64_t r = j;
                        const int64_t i0 = r % n0;
                        r /= n0;
                        const int64_t i1 = r % n1;
                        r /= n1;
                        const int64_t i2 = r % n2;
                        const int64_t i3 = r / n2;
                        s += load_<MODE>(src, base + i0 * s0 + i1 * s1 + i2 * s2 + i3 * s3, real);
                    }
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += shfl_down_(s, off);
            if (lanes == 64) {
                if (lane == 0) add_scaled<MODE>(acc, tm->coeff_re, tm->coeff_im, s);
            } else {
                if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
                __syncthreads();
                if (threadIdx.x == 0) add_scaled<MODE>(acc, tm->coeff_re, tm->coeff_im, ((red[0] + red[1]) + red[2]) + red[3]);
                __syncthreads();
            }
        }
        if (lane == 0 && active) store_<MODE>(dst, dot_(og->dst_strides, o.ndim, idx), acc);
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) trace_weighted_kernel(const Out* __restrict__ outs, const Term* __restrict__ terms, const Item* __restrict__ items)
{
    __shared__ typename Acc<CPLX ? kC128 : kF64>::type red[NT / 64];
    const Item it = items[blockIdx.x];
    const GLOBAL_AS Out* og = (const GLOBAL_AS Out*)(outs + it.out);
    Out o; // (the destination strides stay in memory: they are read once per element)
    o.dst = og->dst, o.ndim = og->ndim, o.first_term = og->first_term, o.n_terms = og->n_terms;
#pragma unroll
    for (int k = 0; k < CYB_MAX_NDIM; ++k) o.shape[k] = og->shape[k];
    if constexpr (CPLX) {
        if (it.lanes == 1)
            lane_regime<kC128>(o, og, terms, it);
        else
            wide_regime<kC128>(o, og, terms, it, red);
    } else {
        if (it.lanes != 1)
            wide_regime<kF64>(o, og, terms, it, red);
        else if (it.mode == kF64x2)
            lane_regime<kF64x2>(o, og, terms, it);
        else
            lane_regime<kF64>(o, og, terms, it);
    }
}

inline bool even_(int64_t v) { return (v & 1) == 0; }
inline bool aligned16_(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool CPLX>
int trace_weighted(cyb_ctx_t ctx, const Out* outs, int64_t n_outs, const Term* terms, int64_t n_terms, const char* who)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n_outs >= 0 && n_terms >= 0 && (n_outs == 0 || outs) && (n_terms == 0 || terms), "%s: bad lists", who);
    if (n_outs == 0) return CYB_OK;
    std::vector<Term> ht(terms, terms + n_terms);
    std::vector<int64_t> addends((size_t)n_terms, 0);
    for (int64_t t = 0; t < n_terms; ++t) {
        Term& tm = ht[(size_t)t];
        CYB_REQUIRE(tm.n_pairs >= 0 && tm.n_pairs <= kPairs, "%s: term %lld: %d traced pairs (at most %d)", who, (long long)t, tm.n_pairs, kPairs);
        CYB_REQUIRE(CPLX || tm.coeff_im == 0.0, "%s: term %lld: a complex coefficient at the float64 entry", who, (long long)t);
        if (!CPLX) tm.src_real = 0;
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
        int lanes, mode;
        int64_t total;
    };
    std::vector<Out> ho(outs, outs + n_outs);
    std::vector<Plan> plan((size_t)n_outs);
    int64_t lane_total = 0;
    for (int64_t i = 0; i < n_outs; ++i) {
        Out& o = ho[(size_t)i];
        CYB_REQUIRE(o.ndim >= 0 && o.ndim <= CYB_MAX_NDIM, "%s: output %lld: ndim %d out of range", who, (long long)i, o.ndim);
        CYB_REQUIRE(o.first_term >= 0 && o.n_terms >= 0 && o.first_term <= n_terms && o.n_terms <= n_terms - o.first_term,
                    "%s: output %lld: bad term range [%lld, +%lld)", who, (long long)i, (long long)o.first_term, (long long)o.n_terms);
        int64_t R = 1;
        for (int k = 0; k < o.ndim; ++k) {
            CYB_REQUIRE(o.shape[k] >= 0, "%s: output %lld: negative extent", who, (long long)i);
            R *= o.shape[k];
        }
        CYB_REQUIRE(R == 0 || o.dst, "%s: output %lld: dst is NULL", who, (long long)i);
        const int last = o.ndim - 1;
        // pairs of elements: the innermost remaining axis is contiguous and everything else keeps 16-byte alignment
        bool x2 = !CPLX && R > 0 && last >= 0 && even_(o.shape[last]) && o.dst_strides[last] == 1 && aligned16_(o.dst);
        for (int k = 0; x2 && k < last; ++k) x2 = o.shape[k] == 1 || even_(o.dst_strides[k]);
        int64_t A = 0;
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t) {
            const Term& tm = ht[(size_t)t];
            CYB_REQUIRE(o.ndim + 2 * tm.n_pairs <= CYB_MAX_NDIM, "%s: term %lld: more than %d source axes", who, (long long)t, CYB_MAX_NDIM);
            CYB_REQUIRE(R == 0 || addends[(size_t)t] == 0 || tm.src, "%s: term %lld: src is NULL", who, (long long)t);
            A += addends[(size_t)t];
            if (x2 && addends[(size_t)t] > 0) {
                x2 = tm.rem_strides[last] == 1 && aligned16_(tm.src);
                for (int k = 0; x2 && k < last; ++k) x2 = o.shape[k] == 1 || even_(tm.rem_strides[k]);
                for (int p = 0; x2 && p < tm.n_pairs; ++p) x2 = tm.pair_extent[p] == 1 || even_(tm.pair_stride[p]);
            }
        }
        // 65536 lanes = one 256-thread workgroup on each of the 256 CUs; 1024 waves = one per SIMD
        int lanes = 1;
        if (A >= 64 && R < 65536) lanes = (A < 4096 || R >= 1024) ? 64 : 256;
        int mode = CPLX ? kC128 : kF64;
        if (lanes == 1 && x2) {
            mode = kF64x2;
            o.shape[last] /= 2;
            R /= 2;
        }
        plan[(size_t)i] = Plan{lanes, mode, R};
        if (lanes == 1) lane_total += R;
    }
    // lane regime: about 2048 workgroups for the launch, at least 4 and at most 256 elements per lane
    int64_t chunk = (lane_total / 2048 + 1023) & ~(int64_t)1023;
    chunk = std::min<int64_t>(std::max<int64_t>(chunk, 4 * NT), 256 * NT);
    std::vector<Item> items;
    for (int64_t i = 0; i < n_outs; ++i) {
        const Plan& p = plan[(size_t)i];
        const int64_t step = p.lanes == 1 ? chunk : NT / p.lanes; // wave: 4 elements (one per wave), group: 1 element per workgroup
        for (int64_t s = 0; s < p.total; s += step)
            items.push_back(Item{(int32_t)i, (int16_t)p.lanes, (int16_t)p.mode, s, std::min(step, p.total - s)});
    }
    return cyb_flat::launch(ctx, who, trace_weighted_kernel<CPLX>, cyb_flat::arrays(ho, ht, items));
}

} // namespace

extern "C" {

int cyb_trace_weighted_f64(cyb_ctx_t ctx, const cyb_trace_weighted_out* outs, int64_t n_outs, const cyb_trace_weighted_term* terms, int64_t n_terms)
{
    return trace_weighted<false>(ctx, outs, n_outs, terms, n_terms, "cyb_trace_weighted_f64");
}

int cyb_trace_weighted_c128(cyb_ctx_t ctx, const cyb_trace_weighted_out* outs, int64_t n_outs, const cyb_trace_weighted_term* terms, int64_t n_terms)
{
    return trace_weighted<true>(ctx, outs, n_outs, terms, n_terms, "cyb_trace_weighted_c128");
}

} // extern "C"
