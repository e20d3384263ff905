// Fusion-tree tensors <-> dense arrays: every region of FusionTreeBackend::to_dense_block, and every tile of
// FusionTreeBackend::from_dense_block, in ONE launch each.
//
// to_dense_block (src/backends/fusion_tree_backend.cpp:1856-1973, helper _get_forest_block_contribution :1532-1604) makes,
// per pair of trees of every forest pair of every coupled block, a zeros, two to_dense_block of trees, tdot, get_item,
// reshape, outer and operator+, then permute_axes, reshape and an accumulating set_item into a dense tensor that was
// zero-filled first.  Here an *output* record is one region of the dense tensor -- the positions of one combination of
// uncoupled sectors (a_1..a_J, b_1..b_K) -- seen as an index space of up to 12 levels (k_1, m_1, ..., one (k, m) per leg: k
// inside the sector's dimension, m inside its multiplicity) in the flat order the caller gives (last level fastest), with
// a destination stride per level.  A *term* record is one contributing (coupled block, tree alpha, tree beta):
//   dst[sum_l x_l sd_l] = sum_t S[s_off_t + sum_l x_l ss_l] * B_t[(first_row_t + sum_l x_l sr_l) * rs_t + (first_col_t + sum_l x_l sc_l) * cs_t]
// S_{alpha beta}[k_a..., k_b...] is the contracted pair of tree tensors (a small TENSOR per term, not a scalar), B_t the
// coupled block read in place.  The regions of all combinations partition the dense tensor: every element has exactly one
// owner, which adds its terms in ascending order in registers; a region without terms is written as zeros.  No zero fill, no
// float atomics, no second pass, bit-identical from run to run.
//
// from_dense_block (:1680-1853, helper _add_forest_block_entries :1606-1677: two tdot, trace_partial, a division, reshape and
// set_item per pair of trees) is the adjoint read stream: an output record is one tile (tree alpha, tree beta) of a coupled
// block with the levels (m_1..m_J, n_1..n_K), a term one dense region:
//   dst[sum_l x_l sd_l] = (sum_t sum_k conj(S[s_off_t + k]) * A_t[sum_l x_l ss_l + sum_j k_j ks_j]) / divisor
// k = (k_1, ..) runs in C order inside the lane (S and the k digits are wave-uniform: scalar loads, scalar arithmetic).
//
// Both directions share the work-item machinery of tree_outer.hip:
//   * host: a record is cut into work items of kMinChunk..kMaxChunk flat units; ONE WAVE owns an item (four items per
//     workgroup, no LDS, no barrier), so one launch balances thousands of tiny regions beside one of tens of MB.  Levels of
//     extent 1 are dropped on the host.
//   * device: a lane keeps a cursor -- the digits and one running offset per stream (destination, S / source, block row,
//     block column).  It decodes its lane offset (below 64: 32-bit divisions) once per item and then advances by the wave's
//     step of 64 units with the precomputed digits of the step and a precomputed correction per wrap of a level:
//     additions and compares only, no division per element.
//   * the lanes run along the flat order of the levels: the caller orders them so that the last level is the contiguous run
//     of the destination (to_dense) or of the source (from_dense).
//   * item, record and term are wave-uniform: their fields travel through scalar loads, the term loop is innermost.
// A lane holds one element: an 8-byte store for float64, a 16-byte store for complex128.
#include "common.h"

#include <algorithm>

namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#define GLOBAL_AS __attribute__((address_space(1)))
#else
#define GLOBAL_AS
#endif

constexpr int NT = 256, WAVE = 64, ITEMS_PER_GROUP = NT / WAVE;
constexpr int NL = CYB_TREE_DENSE_MAX_LEVELS, NK = CYB_TREE_DENSE_MAX_LEGS, NS = 4;
constexpr int64_t kMinChunk = 1024, kMaxChunk = 16384, kTargetItems = 8192; // flat units per work item (multiples of WAVE)
typedef double d2 __attribute__((ext_vector_type(2)));
typedef cyb_tree_to_dense_term FwdTerm;
typedef cyb_tree_from_dense_term BwdTerm;

// streams of a cursor: the destination; to_dense: S, block row, block column; from_dense: the source
enum { kDst = 0, kS = 1, kRow = 2, kCol = 3, kSrc = 1 };

// one output as the kernels read it; the levels are right-aligned, unused ones have extent 1 and strides 0
struct Rec {
    double* dst;
    int64_t first_term, n_terms;
    int32_t ext[NL];
    int32_t step[NL];    // digits of the step of WAVE units
    int64_t st[NS][NL];  // stride of every level in every stream (elements of the stream's own type)
    int64_t wr[NS][NL];  // correction of a stream's offset when level l wraps: st[l - 1] - ext[l] * st[l]
    int64_t step_o[NS];  // increment of a stream's offset per step, before corrections
    // from_dense only: the contracted levels, right-aligned (unused: extent 1, stride 0), and the divisor
    int32_t kext[NK];
    int32_t ktotal, reserved;
    int64_t kst[NK];
    int64_t kwr[NK];     // what the source offset gains when level j wraps: -(kext[j] - 1) * kst[j]
    double divisor;
};

struct Item {
    int32_t rec;
    int32_t reserved;
    int64_t count;   // flat units of this item
    int64_t off[NS]; // stream offsets of its first unit
    int32_t idx[NL]; // digits of its first unit
};

template <int N> struct Cursor {
    int32_t idx[NL];
    int64_t off[N];
};

// c += (digits dg, whose stream offsets are d); every digit below its extent, so a level wraps at most once
template <int N> __host__ __device__ inline void advance(Cursor<N>& c, const Rec& r, const int32_t (&dg)[NL], const int64_t* d)
{
#pragma unroll
    for (int a = 0; a < N; ++a) c.off[a] += d[a];
    int32_t carry = 0;
#pragma unroll
    for (int l = NL - 1; l >= 0; --l) {
        const int32_t i = c.idx[l] + dg[l] + carry;
        const bool w = i >= r.ext[l];
        c.idx[l] = w ? i - r.ext[l] : i;
#pragma unroll
        for (int a = 0; a < N; ++a) c.off[a] += w ? r.wr[a][l] : 0;
        carry = w ? 1 : 0;
    }
}

// the cursor of `lane` at the start of an item
template <int N> __host__ __device__ inline void start(Cursor<N>& c, const Rec& r, const Item& it, int lane)
{
#pragma unroll
    for (int l = 0; l < NL; ++l) c.idx[l] = it.idx[l];
#pragma unroll
    for (int a = 0; a < N; ++a) c.off[a] = it.off[a];
    // lane offset into the item -> digits (below 64: 32-bit divisions, extents above it never divide)
    uint32_t d = (uint32_t)lane;
    int32_t dg[NL];
    int64_t dd[N];
#pragma unroll
    for (int a = 0; a < N; ++a) dd[a] = 0;
#pragma unroll
    for (int l = NL - 1; l >= 0; --l) {
        const uint32_t e32 = r.ext[l] > WAVE ? (uint32_t)WAVE + 1 : (uint32_t)r.ext[l];
        const uint32_t q = d / e32;
        dg[l] = (int32_t)(d - q * e32);
        d = q;
#pragma unroll
        for (int a = 0; a < N; ++a) dd[a] += dg[l] * r.st[a][l];
    }
    advance<N>(c, r, dg, dd);
}

template <bool CPLX> struct Acc { typedef d2 type; };
template <> struct Acc<false> { typedef double type; };

template <bool CPLX> __host__ __device__ inline typename Acc<CPLX>::type zero_()
{
    if constexpr (CPLX) return d2{0.0, 0.0}; else return 0.0;
}

template <bool CPLX> __host__ __device__ inline void store_(double* dst_, int64_t o, typename Acc<CPLX>::type v)
{
    GLOBAL_AS double* dst = (GLOBAL_AS double*)dst_;
    if constexpr (CPLX) *(GLOBAL_AS d2*)(dst + 2 * o) = v; else dst[o] = v;
}

// a value of `p` at element offset o: complex storage, or float64 storage read as it stands
__host__ __device__ inline d2 load_c(const double* p_, int64_t o, bool real)
{
    const GLOBAL_AS double* p = (const GLOBAL_AS double*)p_;
    return real ? d2{p[o], 0.0} : *(const GLOBAL_AS d2*)(p + 2 * o);
}

template <bool CPLX>
__host__ __device__ inline void to_dense_item(const Rec& r, const Item& it, const FwdTerm* __restrict__ terms, const double* __restrict__ stab, int lane)
{
    Cursor<4> c;
    start<4>(c, r, it, lane);
    for (int64_t k = lane; k < it.count; k += WAVE) {
        typename Acc<CPLX>::type acc = zero_<CPLX>();
        for (int64_t t = r.first_term; t < r.first_term + r.n_terms; ++t) {
            const FwdTerm& tm = terms[t];
            const int64_t os = tm.s_off + c.off[kS];
            const int64_t ob = (tm.first_row + c.off[kRow]) * tm.rs + (tm.first_col + c.off[kCol]) * tm.cs;
            if constexpr (CPLX) {
                const d2 s = load_c(stab, os, tm.s_real != 0), b = load_c(tm.block, ob, tm.block_real != 0);
                acc.x += s.x * b.x - s.y * b.y;
                acc.y += s.x * b.y + s.y * b.x;
            } else {
                acc += ((const GLOBAL_AS double*)stab)[os] * ((const GLOBAL_AS double*)tm.block)[ob];
            }
        }
        store_<CPLX>(r.dst, c.off[kDst], acc);
        advance<4>(c, r, r.step, r.step_o);
    }
}

template <bool CPLX>
__host__ __device__ inline void from_dense_item(const Rec& r, const Item& it, const BwdTerm* __restrict__ terms, const double* __restrict__ stab, int lane)
{
    Cursor<2> c;
    start<2>(c, r, it, lane);
    for (int64_t k = lane; k < it.count; k += WAVE) {
        typename Acc<CPLX>::type acc = zero_<CPLX>();
        for (int64_t t = r.first_term; t < r.first_term + r.n_terms; ++t) {
            const BwdTerm& tm = terms[t];
            // the contracted levels in C order: digits and source offset are the same in every lane
            int32_t kd[NK];
#pragma unroll
            for (int j = 0; j < NK; ++j) kd[j] = 0;
            int64_t ko = 0;
            for (int32_t kk = 0; kk < r.ktotal; ++kk) {
                const int64_t os = tm.s_off + kk, oa = c.off[kSrc] + ko;
                if constexpr (CPLX) {
                    const d2 s = load_c(stab, os, tm.s_real != 0), a = load_c(tm.src, oa, tm.src_real != 0);
                    acc.x += s.x * a.x + s.y * a.y;      // conj(s) * a
                    acc.y += s.x * a.y - s.y * a.x;
                } else {
                    acc += ((const GLOBAL_AS double*)stab)[os] * ((const GLOBAL_AS double*)tm.src)[oa];
                }
                bool carry = true;
#pragma unroll
                for (int j = NK - 1; j >= 0; --j) {
                    const bool w = carry && kd[j] + 1 >= r.kext[j];
                    ko += carry ? (w ? r.kwr[j] : r.kst[j]) : 0;
                    kd[j] = carry ? (w ? 0 : kd[j] + 1) : kd[j];
                    carry = w;
                }
            }
        }
        if constexpr (CPLX) acc = d2{acc.x / r.divisor, acc.y / r.divisor}; else acc = acc / r.divisor;
        store_<CPLX>(r.dst, c.off[kDst], acc);
        advance<2>(c, r, r.step, r.step_o);
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) to_dense_kernel(const Rec* __restrict__ recs, const FwdTerm* __restrict__ terms, const Item* __restrict__ items,
                                                      int n_items, const double* __restrict__ stab)
{
    // one wave per item: the index is wave-uniform, and so is everything read through it
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ITEMS_PER_GROUP + threadIdx.x / WAVE));
    if (i >= n_items) return;
    const Item& it = items[i];
    to_dense_item<CPLX>(recs[it.rec], it, terms, stab, threadIdx.x & (WAVE - 1));
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) from_dense_kernel(const Rec* __restrict__ recs, const BwdTerm* __restrict__ terms, const Item* __restrict__ items,
                                                        int n_items, const double* __restrict__ stab)
{
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ITEMS_PER_GROUP + threadIdx.x / WAVE));
    if (i >= n_items) return;
    const Item& it = items[i];
    from_dense_item<CPLX>(recs[it.rec], it, terms, stab, threadIdx.x & (WAVE - 1));
}

// ---- host: records and work items ------------------------------------------------------------------------------------

struct Plan {
    std::vector<Rec> recs;
    std::vector<int64_t> totals;
    std::vector<Item> items;
};

// the levels of one output -> a Rec (levels of extent 1 dropped, the others right-aligned); false: an extent is negative or
// too large.  total: the number of flat units (0: nothing to do)
template <int N>
bool make_rec(Rec& r, int n_levels, const int64_t* ext, const int64_t* const (&strides)[N], int64_t& total)
{
    memset(&r, 0, sizeof(r));
    for (int l = 0; l < NL; ++l) r.ext[l] = 1;
    for (int j = 0; j < NK; ++j) r.kext[j] = 1;
    r.ktotal = 1;
    r.divisor = 1.0;
    total = 1;
    int kept = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (ext[l] < 0 || ext[l] > INT32_MAX / 2) return false;
        if (ext[l] != 0 && total > (INT64_MAX >> 4) / ext[l]) return false;
        total *= ext[l];
        kept += ext[l] != 1;
    }
    if (total == 0) return true;
    int at = NL - kept;
    for (int l = 0; l < n_levels; ++l) {
        if (ext[l] == 1) continue;
        r.ext[at] = (int32_t)ext[l];
        for (int a = 0; a < N; ++a) r.st[a][at] = strides[a][l];
        ++at;
    }
    int64_t s = WAVE;
    for (int l = NL - 1; l >= 0; --l) {
        for (int a = 0; a < N; ++a) r.wr[a][l] = (l > 0 ? r.st[a][l - 1] : 0) - r.ext[l] * r.st[a][l];
        // digits of the step; what is left at the outermost level stays there (a cursor is only read while inside the record)
        r.step[l] = (int32_t)(l > 0 ? s % r.ext[l] : std::min<int64_t>(s, r.ext[0]));
        s = l > 0 ? s / r.ext[l] : 0;
        for (int a = 0; a < N; ++a) r.step_o[a] += r.step[l] * r.st[a][l];
    }
    return true;
}

template <int N> void cut_items(Plan& p)
{
    int64_t grand = 0;
    for (int64_t t : p.totals) grand += t;
    // about kTargetItems waves for a large launch
    int64_t chunk = (grand / kTargetItems + WAVE - 1) / WAVE * WAVE;
    chunk = std::min(std::max(chunk, kMinChunk), kMaxChunk);
    for (size_t i = 0; i < p.recs.size(); ++i) {
        const Rec& r = p.recs[i];
        int first = 0; // the levels in use are the last ones
        while (first < NL && r.ext[first] == 1) ++first;
        // the digits of the chunk; the items of a record follow each other by additions, no division per item
        int32_t cd[NL] = {0};
        int64_t e = chunk;
        for (int l = NL - 1; l >= first; --l) {
            cd[l] = (int32_t)(e % r.ext[l]);
            e /= r.ext[l];
        }
        Item it;
        memset(&it, 0, sizeof(it));
        it.rec = (int32_t)i;
        for (int64_t e0 = 0; e0 < p.totals[i]; e0 += chunk) {
            it.count = std::min(chunk, p.totals[i] - e0);
            for (int a = 0; a < N; ++a) {
                it.off[a] = 0;
                for (int l = first; l < NL; ++l) it.off[a] += it.idx[l] * r.st[a][l];
            }
            p.items.push_back(it);
            int32_t carry = 0;
            for (int l = NL - 1; l >= first; --l) {
                const int32_t v = it.idx[l] + cd[l] + carry;
                carry = v >= r.ext[l] ? 1 : 0;
                it.idx[l] = carry ? v - r.ext[l] : v;
            }
        }
    }
}

#define TD_RANGE(o, i)                                                                                                                   \
    CYB_REQUIRE((o).first_term >= 0 && (o).n_terms >= 0 && (o).first_term <= n_terms && (o).n_terms <= n_terms - (o).first_term,         \
                "%s: output %lld: bad term range [%lld, +%lld)", who, (long long)(i), (long long)(o).first_term, (long long)(o).n_terms)

template <bool CPLX>
int plan_to_dense(Plan& p, std::vector<FwdTerm>& ht, const cyb_tree_to_dense_out* outs, int64_t n_outs, int64_t n_terms, const double* s_table,
                  const char* who)
{
    for (auto& tm : ht)
        if (!CPLX) tm.block_real = tm.s_real = 0;
    for (int64_t i = 0; i < n_outs; ++i) {
        const cyb_tree_to_dense_out& o = outs[i];
        CYB_REQUIRE(o.n_levels >= 0 && o.n_levels <= NL, "%s: output %lld: %d levels, at most %d", who, (long long)i, (int)o.n_levels, NL);
        TD_RANGE(o, i);
        Rec r;
        int64_t total;
        const int64_t* const strides[4] = {o.sd, o.ss, o.sr, o.sc};
        for (int l = 0; l < o.n_levels; ++l) CYB_REQUIRE(o.ext[l] >= 0, "%s: output %lld: negative extent", who, (long long)i);
        CYB_REQUIRE(make_rec<4>(r, o.n_levels, o.ext, strides, total), "%s: output %lld: extent too large", who, (long long)i);
        if (total == 0) continue;
        CYB_REQUIRE(o.dst, "%s: output %lld: dst is NULL", who, (long long)i);
        CYB_REQUIRE(o.n_terms == 0 || s_table, "%s: s_table is NULL", who);
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t) {
            const FwdTerm& tm = ht[(size_t)t];
            CYB_REQUIRE(tm.block, "%s: term %lld: block is NULL", who, (long long)t);
            CYB_REQUIRE(tm.first_row >= 0 && tm.first_col >= 0 && tm.s_off >= 0, "%s: term %lld: negative first_row, first_col or s_off", who,
                        (long long)t);
        }
        r.dst = o.dst, r.first_term = o.first_term, r.n_terms = o.n_terms;
        p.recs.push_back(r);
        p.totals.push_back(total);
    }
    cut_items<4>(p);
    return CYB_OK;
}

template <bool CPLX>
int plan_from_dense(Plan& p, std::vector<BwdTerm>& ht, const cyb_tree_from_dense_out* outs, int64_t n_outs, int64_t n_terms, const double* s_table,
                    const char* who)
{
    for (auto& tm : ht)
        if (!CPLX) tm.src_real = tm.s_real = 0;
    for (int64_t i = 0; i < n_outs; ++i) {
        const cyb_tree_from_dense_out& o = outs[i];
        CYB_REQUIRE(o.n_levels >= 0 && o.n_levels <= NK && o.n_k >= 0 && o.n_k <= NK, "%s: output %lld: %d levels and %d contracted levels, at most %d each",
                    who, (long long)i, (int)o.n_levels, (int)o.n_k, NK);
        TD_RANGE(o, i);
        Rec r;
        int64_t total;
        const int64_t* const strides[2] = {o.sd, o.ss};
        for (int l = 0; l < o.n_levels; ++l) CYB_REQUIRE(o.ext[l] >= 0, "%s: output %lld: negative extent", who, (long long)i);
        CYB_REQUIRE(make_rec<2>(r, o.n_levels, o.ext, strides, total), "%s: output %lld: extent too large", who, (long long)i);
        int64_t ktotal = 1;
        for (int j = 0; j < o.n_k; ++j) {
            CYB_REQUIRE(o.kext[j] >= 0, "%s: output %lld: negative contracted extent", who, (long long)i);
            CYB_REQUIRE(o.kext[j] == 0 || ktotal <= (1 << 30) / o.kext[j], "%s: output %lld: contracted extent too large", who, (long long)i);
            ktotal *= o.kext[j];
        }
        CYB_REQUIRE(o.divisor != 0.0 && o.divisor == o.divisor, "%s: output %lld: the divisor is zero or NaN", who, (long long)i);
        if (total == 0) continue;
        CYB_REQUIRE(o.dst, "%s: output %lld: dst is NULL", who, (long long)i);
        CYB_REQUIRE(o.n_terms == 0 || ktotal == 0 || s_table, "%s: s_table is NULL", who);
        for (int64_t t = o.first_term; t < o.first_term + o.n_terms; ++t) {
            CYB_REQUIRE(ktotal == 0 || ht[(size_t)t].src, "%s: term %lld: src is NULL", who, (long long)t);
            CYB_REQUIRE(ht[(size_t)t].s_off >= 0, "%s: term %lld: negative s_off", who, (long long)t);
        }
        int at = NK - o.n_k;
        for (int j = 0; j < o.n_k; ++j, ++at) {
            r.kext[at] = (int32_t)o.kext[j];
            r.kst[at] = o.ks[j];
            r.kwr[at] = -(o.kext[j] - 1) * o.ks[j];
        }
        r.ktotal = (int32_t)ktotal;
        r.divisor = o.divisor;
        r.dst = o.dst, r.first_term = o.first_term, r.n_terms = o.n_terms;
        p.recs.push_back(r);
        p.totals.push_back(total);
    }
    cut_items<2>(p);
    return CYB_OK;
}

template <typename TermT, typename Kernel>
int launch(cyb_ctx_t ctx, const Plan& p, const std::vector<TermT>& ht, const double* s_table, Kernel kernel, const char* who)
{
    if (p.items.empty()) return CYB_OK;
    CYB_REQUIRE(p.items.size() < ((size_t)1 << 31), "%s: too many work items", who);
    void *d_recs = nullptr, *d_terms = nullptr, *d_items = nullptr;
    CYB_TRY(cyb::upload_packed(ctx, {{p.recs.data(), sizeof(Rec) * p.recs.size(), &d_recs},
                                     {ht.empty() ? (const void*)p.recs.data() : (const void*)ht.data(), ht.empty() ? 8 : sizeof(TermT) * ht.size(), &d_terms},
                                     {p.items.data(), sizeof(Item) * p.items.size(), &d_items}}));
    const unsigned grid = (unsigned)((p.items.size() + ITEMS_PER_GROUP - 1) / ITEMS_PER_GROUP);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), 0, ctx->stream, static_cast<const Rec*>(d_recs), static_cast<const TermT*>(d_terms),
                       static_cast<const Item*>(d_items), (int)p.items.size(), s_table);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

template <bool CPLX>
int tree_to_dense(cyb_ctx_t ctx, const cyb_tree_to_dense_out* outs, int64_t n_outs, const FwdTerm* terms, int64_t n_terms, const double* s_table,
                  const char* who)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n_outs >= 0 && n_terms >= 0 && (n_outs == 0 || outs) && (n_terms == 0 || terms), "%s: bad lists", who);
    if (n_outs == 0) return CYB_OK;
    std::vector<FwdTerm> ht(terms, terms + n_terms);
    Plan p;
    CYB_TRY(plan_to_dense<CPLX>(p, ht, outs, n_outs, n_terms, s_table, who));
    return launch(ctx, p, ht, s_table, to_dense_kernel<CPLX>, who);
}

template <bool CPLX>
int tree_from_dense(cyb_ctx_t ctx, const cyb_tree_from_dense_out* outs, int64_t n_outs, const BwdTerm* terms, int64_t n_terms, const double* s_table,
                    const char* who)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n_outs >= 0 && n_terms >= 0 && (n_outs == 0 || outs) && (n_terms == 0 || terms), "%s: bad lists", who);
    if (n_outs == 0) return CYB_OK;
    std::vector<BwdTerm> ht(terms, terms + n_terms);
    Plan p;
    CYB_TRY(plan_from_dense<CPLX>(p, ht, outs, n_outs, n_terms, s_table, who));
    return launch(ctx, p, ht, s_table, from_dense_kernel<CPLX>, who);
}
} // namespace

extern "C" {

int cyb_tree_to_dense_f64(cyb_ctx_t ctx, const cyb_tree_to_dense_out* outs, int64_t n_outs, const cyb_tree_to_dense_term* terms, int64_t n_terms,
                          const double* s_table)
{
    return tree_to_dense<false>(ctx, outs, n_outs, terms, n_terms, s_table, "cyb_tree_to_dense_f64");
}

int cyb_tree_to_dense_c128(cyb_ctx_t ctx, const cyb_tree_to_dense_out* outs, int64_t n_outs, const cyb_tree_to_dense_term* terms, int64_t n_terms,
                           const double* s_table)
{
    return tree_to_dense<true>(ctx, outs, n_outs, terms, n_terms, s_table, "cyb_tree_to_dense_c128");
}

int cyb_tree_from_dense_f64(cyb_ctx_t ctx, const cyb_tree_from_dense_out* outs, int64_t n_outs, const cyb_tree_from_dense_term* terms, int64_t n_terms,
                            const double* s_table)
{
    return tree_from_dense<false>(ctx, outs, n_outs, terms, n_terms, s_table, "cyb_tree_from_dense_f64");
}

int cyb_tree_from_dense_c128(cyb_ctx_t ctx, const cyb_tree_from_dense_out* outs, int64_t n_outs, const cyb_tree_from_dense_term* terms, int64_t n_terms,
                             const double* s_table)
{
    return tree_from_dense<true>(ctx, outs, n_outs, terms, n_terms, s_table, "cyb_tree_from_dense_c128");
}

} // extern "C"
