// Segment ops: elementwise arithmetic / comparisons, reductions and stream compaction of a LIST of 1-D sector blocks
// ("segments") in ONE launch per call.
//
// The reference works on a DiagonalTensor or a Mask one sector at a time, with host round trips inside the loop:
// diagonal_elementwise_binary (src/backends/abelian.cpp:1596-1619), reduce_DiagonalTensor (:3163-3173), diagonal_all /
// diagonal_any (:726-738), diagonal_to_mask (:1707-1728: any, sum_all and to_numpy per sector), mask_binary_operand
// (:2410-2440) and mask_unary_operand (:2705-2728).  Here the host cuts the list into work items and one kernel serves all
// of them.  The owner of a segment is chosen from its length n alone:
//   * lanes (16 lanes, 16 segments per workgroup):  n <= 64     -- a list of many short segments costs 1/16 workgroup each
//   * wave  (64 lanes, 4 segments per workgroup):   n <= 1024
//   * group (one 256-thread workgroup):             n <= 16384
//   * chunks (one workgroup per 16384 elements):    above; chunk starts are multiples of 16384 whatever the chip
// Reductions: a lane adds the element PAIRS (2p, 2p + 1), p = lane, lane + L, ... in ascending order, the lanes are folded
// by a shuffle tree of fixed shape, the four waves of a workgroup are added by lane 0 in wave order, and the chunk partials
// of a long segment are added in chunk order by the workgroup that draws the last integer ticket.  No float atomics; the
// order depends on n only, not on the alignment (an aligned pair is one 16-byte load, an unaligned one two 8-byte loads of
// the same two elements), the number of CUs or the rest of the list.  Compaction ranks the kept elements of a wave with a
// 64-bit __ballot and popcounts, adds the wave counts of a round in wave order and the rounds in ascending order.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int NT = 256;
constexpr int64_t kLanesMax = 64;    // n <= 64: 16 lanes
constexpr int64_t kWaveMax = 1024;   // n <= 1024: one wave
constexpr int64_t kChunk = 16384;    // n <= 16384: one workgroup; above: one workgroup per chunk of 16384
constexpr int R_LANES = 0, R_WAVE = 1, R_GROUP = 2;

typedef double d2 __attribute__((ext_vector_type(2)));

struct Item {
    int32_t regime;
    int32_t first;  // R_LANES / R_WAVE: first entry of `order` of this workgroup; R_GROUP: the segment
    int32_t count;  // R_LANES / R_WAVE: number of segments of this workgroup (<= 16 / <= 4)
    int32_t chunk;  // R_GROUP: chunk of the segment
    int64_t parts;  // R_GROUP of a multi-chunk segment: first entry of the partial table; else -1
    int64_t ticket; // index of the ticket counter of a multi-chunk segment
};

struct Plan {
    std::vector<int32_t> order;
    std::vector<Item> items;
    int64_t n_parts = 0, n_multi = 0;
};

inline bool kind_ok(int k) { return k >= CYB_SEG_ABSENT && k <= CYB_SEG_BOOL; }

// validates the operand `a` side of every record (and b / out for the binary entry) and builds the work items
int build_plan(const cyb_seg_rec* recs, int64_t n, bool binary, bool skip_empty, Plan& plan, const char* who)
{
    CYB_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && (n == 0 || recs), "%s: bad list", who);
    std::vector<int32_t> lanes, waves;
    for (int64_t s = 0; s < n; ++s) {
        const cyb_seg_rec& r = recs[s];
        CYB_REQUIRE(r.n >= 0, "%s: segment %lld: negative length", who, (long long)s);
        CYB_REQUIRE(kind_ok(r.a_kind), "%s: segment %lld: bad kind of a", who, (long long)s);
        CYB_REQUIRE(r.n == 0 || r.a_kind == CYB_SEG_ABSENT || r.a, "%s: segment %lld: a is NULL", who, (long long)s);
        CYB_REQUIRE(r.a_kind == CYB_SEG_BOOL || ((uintptr_t)r.a & 7) == 0, "%s: segment %lld: a is misaligned", who, (long long)s);
        if (binary) {
            CYB_REQUIRE(kind_ok(r.b_kind), "%s: segment %lld: bad kind of b", who, (long long)s);
            CYB_REQUIRE(r.n == 0 || r.b_kind == CYB_SEG_ABSENT || r.b, "%s: segment %lld: b is NULL", who, (long long)s);
            CYB_REQUIRE(r.b_kind == CYB_SEG_BOOL || ((uintptr_t)r.b & 7) == 0, "%s: segment %lld: b is misaligned", who, (long long)s);
            CYB_REQUIRE(r.out_kind >= CYB_SEG_F64 && r.out_kind <= CYB_SEG_BOOL, "%s: segment %lld: bad kind of out", who, (long long)s);
            CYB_REQUIRE(r.n == 0 || r.out, "%s: segment %lld: out is NULL", who, (long long)s);
            CYB_REQUIRE(r.out_kind == CYB_SEG_BOOL || ((uintptr_t)r.out & 7) == 0, "%s: segment %lld: out is misaligned", who, (long long)s);
        }
        if (r.n == 0 && skip_empty) continue;
        if (r.n <= kLanesMax) {
            lanes.push_back((int32_t)s);
        } else if (r.n <= kWaveMax) {
            waves.push_back((int32_t)s);
        } else {
            const int64_t nc = cdiv64(r.n, kChunk);
            CYB_REQUIRE(nc < (int64_t(1) << 31), "%s: segment %lld is too long", who, (long long)s);
            const bool multi = nc > 1;
            for (int64_t c = 0; c < nc; ++c)
                plan.items.push_back(Item{R_GROUP, (int32_t)s, 1, (int32_t)c, multi ? plan.n_parts : -1, multi ? plan.n_multi : -1});
            if (multi) plan.n_parts += nc, plan.n_multi += 1;
        }
    }
    for (size_t i = 0; i < lanes.size(); i += 16)
        plan.items.push_back(Item{R_LANES, (int32_t)(plan.order.size() + i), (int32_t)std::min<size_t>(16, lanes.size() - i), 0, -1, -1});
    plan.order.insert(plan.order.end(), lanes.begin(), lanes.end());
    const size_t w0 = plan.order.size();
    for (size_t i = 0; i < waves.size(); i += 4)
        plan.items.push_back(Item{R_WAVE, (int32_t)(w0 + i), (int32_t)std::min<size_t>(4, waves.size() - i), 0, -1, -1});
    plan.order.insert(plan.order.end(), waves.begin(), waves.end());
    return CYB_OK;
}

// ---------------------------------------------------------------------------------------------------------- loads / stores

__device__ inline d2 load1(const void* p, int kind, int64_t e)
{
    switch (kind) {
    case CYB_SEG_F64: return d2{((const double*)p)[e], 0.0};
    case CYB_SEG_C128: {
        const double* q = (const double*)p + 2 * e;
        if (((uintptr_t)q & 15) == 0) return *(const d2*)q;
        return d2{q[0], q[1]};
    }
    case CYB_SEG_BOOL: return d2{((const uint8_t*)p)[e] ? 1.0 : 0.0, 0.0};
    default: return d2{0.0, 0.0};
    }
}

// elements e and e + 1 (e even relative to the segment start); `vec`: float64 operand whose pairs are 16-byte aligned
__device__ inline void load2(const void* p, int kind, bool vec, int64_t e, bool has1, d2& v0, d2& v1)
{
    if (vec && has1) {
        const d2 t = *(const d2*)((const double*)p + e);
        v0 = d2{t.x, 0.0};
        v1 = d2{t.y, 0.0};
        return;
    }
    v0 = load1(p, kind, e);
    v1 = has1 ? load1(p, kind, e + 1) : d2{0.0, 0.0};
}

__device__ inline bool pair_aligned(const void* p, int kind) { return kind == CYB_SEG_F64 && ((uintptr_t)p & 15) == 0; }

struct Range {
    int64_t lo, hi; // elements of the segment this owner covers (lo even)
    int lane, L;    // my lane in the owner and the owner's lane count
};

// the owner of this thread: segment record index (or -1) and element range
__device__ inline int owner_of(const Item& it, const int32_t* __restrict__ order, const cyb_seg_rec* __restrict__ recs, Range& rg)
{
    const int tid = threadIdx.x;
    if (it.regime == R_GROUP) {
        const int64_t n = recs[it.first].n;
        rg.lo = (int64_t)it.chunk * kChunk;
        rg.hi = rg.lo + kChunk < n ? rg.lo + kChunk : n;
        rg.lane = tid, rg.L = NT;
        return it.first;
    }
    const int L = it.regime == R_LANES ? 16 : 64;
    const int g = tid / L;
    rg.lane = tid % L, rg.L = L, rg.lo = 0, rg.hi = 0;
    if (g >= it.count) return -1;
    const int seg = order[it.first + g];
    rg.hi = recs[seg].n;
    return seg;
}

// ---------------------------------------------------------------------------------------------------------- binary

__device__ inline d2 apply(d2 a, d2 b, int op, bool cplx)
{
    switch (op) {
    case CYB_SEG_ADD: return a + b;
    case CYB_SEG_SUB: return a - b;
    case CYB_SEG_MUL:
        if (!cplx) return d2{a.x * b.x, 0.0};
        return d2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
    case CYB_SEG_DIV: {
        if (!cplx) return d2{a.x / b.x, 0.0};
        if (b.y == 0.0) return d2{a.x / b.x, a.y / b.x}; // (a real divisor: one correctly rounded division per component)
        const double d = b.x * b.x + b.y * b.y; // a conj(b) / |b|^2
        return d2{(a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d};
    }
    case CYB_SEG_LT: return d2{a.x < b.x ? 1.0 : 0.0, 0.0};
    case CYB_SEG_LE: return d2{a.x <= b.x ? 1.0 : 0.0, 0.0};
    case CYB_SEG_GT: return d2{a.x > b.x ? 1.0 : 0.0, 0.0};
    case CYB_SEG_GE: return d2{a.x >= b.x ? 1.0 : 0.0, 0.0};
    case CYB_SEG_EQ: return d2{(a.x == b.x && a.y == b.y) ? 1.0 : 0.0, 0.0};
    case CYB_SEG_NE: return d2{(a.x != b.x || a.y != b.y) ? 1.0 : 0.0, 0.0};
    default: {
        const bool ta = a.x != 0.0 || a.y != 0.0, tb = b.x != 0.0 || b.y != 0.0;
        const bool r = op == CYB_SEG_AND ? (ta && tb) : op == CYB_SEG_OR ? (ta || tb) : op == CYB_SEG_XOR ? (ta != tb) : !ta;
        return d2{r ? 1.0 : 0.0, 0.0};
    }
    }
}

__device__ inline void store1(void* p, int kind, int64_t e, d2 v)
{
    if (kind == CYB_SEG_F64) {
        ((double*)p)[e] = v.x;
    } else if (kind == CYB_SEG_C128) {
        double* q = (double*)p + 2 * e;
        if (((uintptr_t)q & 15) == 0)
            *(d2*)q = v;
        else
            q[0] = v.x, q[1] = v.y;
    } else {
        ((uint8_t*)p)[e] = v.x != 0.0 ? 1 : 0;
    }
}

__global__ void __launch_bounds__(NT) seg_binary_kernel(const cyb_seg_rec* __restrict__ recs, const int32_t* __restrict__ order,
                                                        const Item* __restrict__ items, int op, int use_scalar, double s_re, double s_im)
{
    const Item it = items[blockIdx.x];
    Range rg;
    const int seg = owner_of(it, order, recs, rg);
    if (seg < 0) return;
    const cyb_seg_rec r = recs[seg];
    const bool cplx = r.out_kind == CYB_SEG_C128 || r.a_kind == CYB_SEG_C128 || r.b_kind == CYB_SEG_C128 || (use_scalar && s_im != 0.0);
    const bool va = pair_aligned(r.a, r.a_kind), vb = !use_scalar && pair_aligned(r.b, r.b_kind);
    const bool vo = r.out_kind == CYB_SEG_F64 && ((uintptr_t)r.out & 15) == 0;
    const d2 sc = d2{s_re, s_im};
    for (int64_t e = rg.lo + 2 * (int64_t)rg.lane; e < rg.hi; e += 2 * (int64_t)rg.L) {
        const bool has1 = e + 1 < rg.hi;
        d2 a0, a1, b0 = sc, b1 = sc;
        load2(r.a, r.a_kind, va, e, has1, a0, a1);
        if (!use_scalar) load2(r.b, r.b_kind, vb, e, has1, b0, b1);
        const d2 c0 = apply(a0, b0, op, cplx), c1 = apply(a1, b1, op, cplx);
        if (vo && has1) {
            *(d2*)((double*)r.out + e) = d2{c0.x, c1.x};
        } else {
            store1(r.out, r.out_kind, e, c0);
            if (has1) store1(r.out, r.out_kind, e + 1, c1);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- reduce

__device__ inline d2 red_ident(int op)
{
    return op == CYB_SEG_MAX ? d2{-INFINITY, 0.0} : op == CYB_SEG_MIN ? d2{INFINITY, 0.0} : d2{0.0, 0.0};
}

__device__ inline d2 red_comb(d2 a, d2 b, int op)
{
    if (op == CYB_SEG_MAX) return d2{fmax(a.x, b.x), 0.0};
    if (op == CYB_SEG_MIN) return d2{fmin(a.x, b.x), 0.0};
    return a + b;
}

__device__ inline d2 red_term(d2 v, int kind, int op, int pre, double param)
{
    switch (pre) {
    case CYB_SEG_PRE_ABS: v = d2{kind == CYB_SEG_C128 ? hypot(v.x, v.y) : fabs(v.x), 0.0}; break;
    case CYB_SEG_PRE_SQUARE: v = d2{v.x * v.x, 0.0}; break;
    case CYB_SEG_PRE_XLOGX: v = d2{v.x > param ? v.x * log(v.x) : 0.0, 0.0}; break;
    case CYB_SEG_PRE_POW: // (x ** 0.5 as Block::pow computes it: a correctly rounded square root, blockops.hip pow_exactish)
        v = d2{param == 0.5 ? (v.x == -INFINITY ? INFINITY : sqrt(v.x) + 0.0) : pow(v.x, param), 0.0};
        break;
    default: break;
    }
    if (op == CYB_SEG_COUNT) return d2{(v.x != 0.0 || v.y != 0.0) ? 1.0 : 0.0, 0.0};
    return v;
}

__device__ inline d2 shfl_down2(d2 v, int off, int width) { return d2{__shfl_down(v.x, off, width), __shfl_down(v.y, off, width)}; }

__global__ void __launch_bounds__(NT) seg_reduce_kernel(const cyb_seg_rec* __restrict__ recs, const int32_t* __restrict__ order,
                                                        const Item* __restrict__ items, int op, int pre, double param,
                                                        double* __restrict__ result, double* parts, unsigned int* tickets)
{
    __shared__ d2 red[NT / 64];
    __shared__ int last;
    const Item it = items[blockIdx.x];
    Range rg;
    const int seg = owner_of(it, order, recs, rg);
    d2 acc = red_ident(op);
    if (seg >= 0) {
        const cyb_seg_rec r = recs[seg];
        const bool va = pair_aligned(r.a, r.a_kind);
        for (int64_t e = rg.lo + 2 * (int64_t)rg.lane; e < rg.hi; e += 2 * (int64_t)rg.L) {
            const bool has1 = e + 1 < rg.hi;
            d2 v0, v1;
            load2(r.a, r.a_kind, va, e, has1, v0, v1);
            acc = red_comb(acc, red_term(v0, r.a_kind, op, pre, param), op);
            if (has1) acc = red_comb(acc, red_term(v1, r.a_kind, op, pre, param), op);
        }
    }
    if (it.regime == R_LANES) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) acc = red_comb(acc, shfl_down2(acc, off, 16), op);
        if (seg >= 0 && rg.lane == 0) result[2 * seg] = acc.x, result[2 * seg + 1] = acc.y;
        return;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = red_comb(acc, shfl_down2(acc, off, 64), op);
    if (it.regime == R_WAVE) {
        if (seg >= 0 && rg.lane == 0) result[2 * seg] = acc.x, result[2 * seg + 1] = acc.y;
        return;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (it.parts < 0) {
        if (threadIdx.x == 0) {
            const d2 t = red_comb(red_comb(red_comb(red[0], red[1], op), red[2], op), red[3], op);
            result[2 * seg] = t.x, result[2 * seg + 1] = t.y;
        }
        return;
    }
    // one chunk of a long segment: publish the partial, draw a ticket; the last workgroup adds the partials in chunk order
    const int64_t n_chunks = (recs[seg].n + kChunk - 1) / kChunk;
    if (threadIdx.x == 0) {
        const d2 t = red_comb(red_comb(red_comb(red[0], red[1], op), red[2], op), red[3], op);
        double* mine = parts + 2 * (it.parts + it.chunk);
        __hip_atomic_store(mine, t.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + 1, t.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const unsigned int ticket = atomicAdd(tickets + it.ticket, 1u);
        last = ticket == (unsigned int)(n_chunks - 1);
        if (last) {
            __threadfence();
            d2 tot = red_ident(op);
            for (int64_t c = 0; c < n_chunks; ++c) {
                const double* p = parts + 2 * (it.parts + c);
                const d2 v = d2{__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                                __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)};
                tot = red_comb(tot, v, op);
            }
            result[2 * seg] = tot.x, result[2 * seg + 1] = tot.y;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- compact

__device__ inline bool flag_at(const cyb_seg_rec& r, int64_t e)
{
    switch (r.a_kind) {
    case CYB_SEG_BOOL: return ((const uint8_t*)r.a)[e] != 0;
    case CYB_SEG_F64: return ((const double*)r.a)[e] != 0.0;
    case CYB_SEG_C128: return ((const double*)r.a)[2 * e] != 0.0 || ((const double*)r.a)[2 * e + 1] != 0.0;
    default: return false;
    }
}

__global__ void __launch_bounds__(NT) seg_compact_kernel(const cyb_seg_rec* __restrict__ recs, const int32_t* __restrict__ order,
                                                         const Item* __restrict__ items, const int64_t* __restrict__ offs,
                                                         int64_t* __restrict__ keep_idx, int64_t* __restrict__ counts)
{
    __shared__ int64_t wcount[NT / 64];
    const Item it = items[blockIdx.x];
    Range rg;
    const int seg = owner_of(it, order, recs, rg);
    const int wlane = threadIdx.x & 63;
    const uint64_t below = wlane ? (~uint64_t(0) >> (64 - wlane)) : 0;

    if (it.regime != R_GROUP) {
        // 16 lanes or one wave per segment: every lane of the wave takes part in the ballot, each owner reads its own field
        const int L = rg.L;
        const int shift = it.regime == R_LANES ? (wlane & ~15) : 0;
        const uint64_t field = it.regime == R_LANES ? uint64_t(0xFFFF) : ~uint64_t(0);
        // (uniform trip count over the wave: the longest segment of the wave's owners)
        int64_t n_max = seg >= 0 ? rg.hi : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int64_t o = __shfl_xor(n_max, off);
            n_max = o > n_max ? o : n_max;
        }
        int64_t base = 0;
        const cyb_seg_rec r = recs[seg >= 0 ? seg : 0];
        int64_t* dst = keep_idx + (seg >= 0 ? offs[seg] : 0);
        for (int64_t e0 = 0; e0 < n_max; e0 += L) {
            const int64_t e = e0 + rg.lane;
            const bool keep = seg >= 0 && e < rg.hi && flag_at(r, e);
            const uint64_t mine = (__ballot(keep) >> shift) & field;
            if (keep) dst[base + __popcll(mine & (below >> shift))] = e;
            base += __popcll(mine);
        }
        if (seg >= 0 && rg.lane == 0) counts[seg] = base;
        return;
    }

    const cyb_seg_rec r = recs[seg];
    // kept elements before this chunk: counted again by this workgroup (integers: any order)
    int64_t before = 0;
    for (int64_t e = threadIdx.x; e < rg.lo; e += NT) before += flag_at(r, e) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    if (wlane == 0) wcount[threadIdx.x >> 6] = before;
    __syncthreads();
    int64_t base = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    __syncthreads();
    int64_t* dst = keep_idx + offs[seg];
    const int w = threadIdx.x >> 6;
    for (int64_t e0 = rg.lo; e0 < rg.hi; e0 += NT) {
        const int64_t e = e0 + threadIdx.x;
        const bool keep = e < rg.hi && flag_at(r, e);
        const uint64_t mine = __ballot(keep);
        if (wlane == 0) wcount[w] = __popcll(mine);
        __syncthreads();
        int64_t wbase = base;
        for (int k = 0; k < w; ++k) wbase += wcount[k];
        if (keep) dst[wbase + __popcll(mine & below)] = e;
        base += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
    if (threadIdx.x == 0 && rg.hi == r.n) counts[seg] = base;
}

// the records, the segment order and the work items in one upload
int upload_plan(cyb_ctx_t ctx, const cyb_seg_rec* recs, int64_t n, const Plan& plan, const std::vector<int64_t>* offs, void** d_recs,
                void** d_order, void** d_items, void** d_offs)
{
    static const int32_t none = 0;
    void* unused = nullptr;
    return cyb::upload_packed(ctx, {{recs, sizeof(cyb_seg_rec) * (size_t)n, d_recs},
                                    {plan.order.empty() ? (const void*)&none : (const void*)plan.order.data(),
                                     plan.order.empty() ? sizeof(none) : sizeof(int32_t) * plan.order.size(), d_order},
                                    {plan.items.data(), sizeof(Item) * plan.items.size(), d_items},
                                    {offs ? (const void*)offs->data() : (const void*)&none, offs ? sizeof(int64_t) * offs->size() : sizeof(none),
                                     offs ? d_offs : &unused}});
}

} // namespace

extern "C" {

int cyb_seg_binary(cyb_ctx_t ctx, const cyb_seg_rec* recs, int64_t n_segs, int32_t op, int32_t use_scalar, double scalar_re, double scalar_im)
{
    const char* who = "cyb_seg_binary";
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(op >= 0 && op < CYB_SEG_N_OPS, "%s: unknown op %d", who, op);
    Plan plan;
    CYB_TRY(build_plan(recs, n_segs, true, true, plan, who));
    for (int64_t s = 0; s < n_segs; ++s) {
        const cyb_seg_rec& r = recs[s];
        const bool cplx = r.a_kind == CYB_SEG_C128 || (!use_scalar && r.b_kind == CYB_SEG_C128) || (use_scalar && scalar_im != 0.0);
        if (op <= CYB_SEG_DIV) // (a real result may be written as complex128: one dtype for all sectors of a complex diagonal)
            CYB_REQUIRE(r.out_kind == CYB_SEG_C128 || (r.out_kind == CYB_SEG_F64 && !cplx), "%s: segment %lld: an arithmetic op writes %s", who,
                        (long long)s, cplx ? "complex128" : "float64 or complex128");
        else
            CYB_REQUIRE(r.out_kind == CYB_SEG_BOOL, "%s: segment %lld: comparisons and logical ops write bool", who, (long long)s);
        if (op >= CYB_SEG_LT && op <= CYB_SEG_GE) CYB_REQUIRE(!cplx, "%s: segment %lld: complex numbers are not ordered", who, (long long)s);
    }
    if (plan.items.empty()) return CYB_OK;
    void *d_recs = nullptr, *d_order = nullptr, *d_items = nullptr;
    CYB_TRY(upload_plan(ctx, recs, n_segs, plan, nullptr, &d_recs, &d_order, &d_items, nullptr));
    hipLaunchKernelGGL(seg_binary_kernel, dim3((unsigned)plan.items.size()), dim3(NT), 0, ctx->stream, static_cast<const cyb_seg_rec*>(d_recs),
                       static_cast<const int32_t*>(d_order), static_cast<const Item*>(d_items), (int)op, (int)(use_scalar != 0), scalar_re, scalar_im);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_seg_reduce(cyb_ctx_t ctx, const cyb_seg_rec* recs, int64_t n_segs, int32_t op, int32_t pre, double param, double* result_dev)
{
    const char* who = "cyb_seg_reduce";
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(op >= 0 && op < CYB_SEG_N_REDUCE, "%s: unknown reduction %d", who, op);
    CYB_REQUIRE(pre >= 0 && pre < CYB_SEG_N_PRE, "%s: unknown pre-map %d", who, pre);
    Plan plan;
    CYB_TRY(build_plan(recs, n_segs, false, false, plan, who));
    if (n_segs == 0) return CYB_OK;
    CYB_REQUIRE(result_dev && ((uintptr_t)result_dev & 7) == 0, "%s: result_dev is NULL or misaligned", who);
    for (int64_t s = 0; s < n_segs; ++s) {
        const int k = recs[s].a_kind;
        CYB_REQUIRE(k != CYB_SEG_C128 || (pre <= CYB_SEG_PRE_ABS && (op == CYB_SEG_SUM || op == CYB_SEG_COUNT || pre == CYB_SEG_PRE_ABS)),
                    "%s: segment %lld: this reduction / pre-map takes real segments", who, (long long)s);
    }
    void *d_recs = nullptr, *d_order = nullptr, *d_items = nullptr, *scratch = nullptr;
    double* parts = nullptr;
    unsigned int* tickets = nullptr;
    if (plan.n_multi) {
        const size_t part_bytes = sizeof(double) * 2 * (size_t)plan.n_parts;
        CYB_TRY(ctx->workspace(part_bytes + sizeof(unsigned int) * (size_t)plan.n_multi, &scratch, 6));
        parts = static_cast<double*>(scratch);
        tickets = reinterpret_cast<unsigned int*>(static_cast<char*>(scratch) + part_bytes);
        CYB_HIP(hipMemsetAsync(tickets, 0, sizeof(unsigned int) * (size_t)plan.n_multi, ctx->stream));
    }
    CYB_TRY(upload_plan(ctx, recs, n_segs, plan, nullptr, &d_recs, &d_order, &d_items, nullptr));
    hipLaunchKernelGGL(seg_reduce_kernel, dim3((unsigned)plan.items.size()), dim3(NT), 0, ctx->stream, static_cast<const cyb_seg_rec*>(d_recs),
                       static_cast<const int32_t*>(d_order), static_cast<const Item*>(d_items), (int)op, (int)pre, param, result_dev, parts, tickets);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_seg_compact(cyb_ctx_t ctx, const cyb_seg_rec* recs, int64_t n_segs, int64_t* keep_idx_dev, int64_t* counts_dev)
{
    const char* who = "cyb_seg_compact";
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    Plan plan;
    CYB_TRY(build_plan(recs, n_segs, false, false, plan, who));
    if (n_segs == 0) return CYB_OK;
    std::vector<int64_t> offs((size_t)n_segs);
    int64_t tot = 0;
    for (int64_t s = 0; s < n_segs; ++s) offs[(size_t)s] = tot, tot += recs[s].n;
    CYB_REQUIRE(counts_dev && ((uintptr_t)counts_dev & 7) == 0, "%s: counts_dev is NULL or misaligned", who);
    CYB_REQUIRE(tot == 0 || (keep_idx_dev && ((uintptr_t)keep_idx_dev & 7) == 0), "%s: keep_idx_dev is NULL or misaligned", who);
    void *d_recs = nullptr, *d_order = nullptr, *d_items = nullptr, *d_offs = nullptr;
    CYB_TRY(upload_plan(ctx, recs, n_segs, plan, &offs, &d_recs, &d_order, &d_items, &d_offs));
    hipLaunchKernelGGL(seg_compact_kernel, dim3((unsigned)plan.items.size()), dim3(NT), 0, ctx->stream, static_cast<const cyb_seg_rec*>(d_recs),
                       static_cast<const int32_t*>(d_order), static_cast<const Item*>(d_items), static_cast<const int64_t*>(d_offs), keep_idx_dev,
                       counts_dev);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

} // extern "C"
