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
// Both directions use the one-wave work items and the cursor of wave_items.h:
//   * a cursor has one running offset per stream (destination, S / source, block row, block column).  Levels of extent 1
//     are dropped on the host.
//   * the lanes run along the flat order of the levels: the caller orders them so that the last level is the contiguous run
//     of the destination (to_dense) or of the source (from_dense).
//   * item, record and term are wave-uniform: their fields travel through scalar loads, the term loop is innermost.
// A lane holds one element: an 8-byte store for float64, a 16-byte store for complex128.
#include "wave_items.h"

namespace {

using namespace cyb_items;
constexpr int NL = CYB_TREE_DENSE_MAX_LEVELS, NK = CYB_TREE_DENSE_MAX_LEGS;
typedef cyb_tree_to_dense_term FwdTerm;
typedef cyb_tree_from_dense_term BwdTerm;

// streams of a cursor: the destination; to_dense: S, block row, block column; from_dense: the source
enum { kDst = 0, kS = 1, kRow = 2, kCol = 3, kSrc = 1 };

// one output as the kernels read it (strides in elements of the stream's own type); the levels are right-aligned, and the
// kernels walk the unused ones (extent 1, strides 0) too
struct FwdRec {
    double* dst;
    int64_t first_term, n_terms;
    Levels<NL, 4> lv;
};
struct BwdRec {
    double* dst;
    int64_t first_term, n_terms;
    Levels<NL, 2> lv;
    // the contracted levels, right-aligned (unused: extent 1, stride 0), and the divisor
    int32_t kext[NK];
    int32_t ktotal, reserved;
    int64_t kst[NK];
    int64_t kwr[NK];     // what the source offset gains when level j wraps: -(kext[j] - 1) * kst[j]
    double divisor;
};
typedef cyb_items::Item<NL, 4> FwdItem;
typedef cyb_items::Item<NL, 2> BwdItem;

template <bool CPLX> constexpr int mode_ = CPLX ? kC128 : kF64;

template <bool CPLX>
__device__ inline void to_dense_item(const FwdRec& r, const FwdItem& it, const FwdTerm* __restrict__ terms, const double* __restrict__ stab, int lane)
{
    Cursor<NL, 4> c;
    start(c, r.lv, it.at, lane, 0);
    for (int64_t k = lane; k < it.count; k += WAVE) {
        typename Val<mode_<CPLX>>::type acc = zero_<mode_<CPLX>>();
        for (int64_t t = r.first_term; t < r.first_term + r.n_terms; ++t) {
            const FwdTerm& tm = terms[t];
            const int64_t os = tm.s_off + c.off[kS];
            const int64_t ob = (tm.first_row + c.off[kRow]) * tm.rs + (tm.first_col + c.off[kCol]) * tm.cs;
            if constexpr (CPLX) {
                const d2 s = load_c(stab, os, tm.s_real != 0), b = load_c(tm.block, ob, tm.block_real != 0);
                acc.x += s.x * b.x - s.y * b.y;
                acc.y += s.x * b.y + s.y * b.x;
            } else {
                acc += load_f64(stab, os) * load_f64(tm.block, ob);
            }
        }
        store_<mode_<CPLX>>(r.dst, c.off[kDst], acc);
        advance(c, r.lv, r.lv.step, r.lv.step_o, 0);
    }
}

template <bool CPLX>
__device__ inline void from_dense_item(const BwdRec& r, const BwdItem& it, const BwdTerm* __restrict__ terms, const double* __restrict__ stab, int lane)
{
    Cursor<NL, 2> c;
    start(c, r.lv, it.at, lane, 0);
    for (int64_t k = lane; k < it.count; k += WAVE) {
        typename Val<mode_<CPLX>>::type acc = zero_<mode_<CPLX>>();
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
                    acc += load_f64(stab, os) * load_f64(tm.src, oa);
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
        store_<mode_<CPLX>>(r.dst, c.off[kDst], acc);
        advance(c, r.lv, r.lv.step, r.lv.step_o, 0);
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) to_dense_kernel(const FwdRec* __restrict__ recs, const FwdTerm* __restrict__ terms,
                                                      const FwdItem* __restrict__ items, int n_items, const double* __restrict__ stab)
{
    int i, lane;
    if (!my_item(i, lane, n_items)) return;
    const FwdItem& it = items[i];
    to_dense_item<CPLX>(recs[it.rec], it, terms, stab, lane);
}

template <bool CPLX>
__global__ void __launch_bounds__(NT) from_dense_kernel(const BwdRec* __restrict__ recs, const BwdTerm* __restrict__ terms,
                                                        const BwdItem* __restrict__ items, int n_items, const double* __restrict__ stab)
{
    int i, lane;
    if (!my_item(i, lane, n_items)) return;
    const BwdItem& it = items[i];
    from_dense_item<CPLX>(recs[it.rec], it, terms, stab, lane);
}

// ---- host: records and work items ------------------------------------------------------------------------------------

// the levels of one output -> a level table (levels of extent 1 dropped, the others right-aligned); false: an extent is
// negative or too large.  total: the number of flat units (0: nothing to do)
template <int N> bool make_levels(Levels<NL, N>& t, int n_levels, const int64_t* ext, const int64_t* const (&strides)[N], int64_t& total)
{
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
        t.ext[at] = (int32_t)ext[l];
        for (int a = 0; a < N; ++a) t.st[a][at] = strides[a][l];
        ++at;
    }
    set_steps(t, NL - kept);
    return true;
}

template <bool CPLX>
int plan_to_dense(std::vector<FwdRec>& recs, std::vector<int64_t>& totals, std::vector<FwdTerm>& ht, const cyb_tree_to_dense_out* outs, int64_t n_outs,
                  int64_t n_terms, const double* s_table, const char* who)
{
    for (auto& tm : ht)
        if (!CPLX) tm.block_real = tm.s_real = 0;
    for (int64_t i = 0; i < n_outs; ++i) {
        const cyb_tree_to_dense_out& o = outs[i];
        CYB_REQUIRE(o.n_levels >= 0 && o.n_levels <= NL, "%s: output %lld: %d levels, at most %d", who, (long long)i, (int)o.n_levels, NL);
        CYB_REQUIRE_TERM_RANGE(who, i, o, n_terms);
        FwdRec r;
        memset(&r, 0, sizeof(r));
        int64_t total;
        const int64_t* const strides[4] = {o.sd, o.ss, o.sr, o.sc};
        for (int l = 0; l < o.n_levels; ++l) CYB_REQUIRE(o.ext[l] >= 0, "%s: output %lld: negative extent", who, (long long)i);
        CYB_REQUIRE(make_levels(r.lv, o.n_levels, o.ext, strides, total), "%s: output %lld: extent too large", who, (long long)i);
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
        recs.push_back(r);
        totals.push_back(total);
    }
    return CYB_OK;
}

template <bool CPLX>
int plan_from_dense(std::vector<BwdRec>& recs, std::vector<int64_t>& totals, std::vector<BwdTerm>& ht, const cyb_tree_from_dense_out* outs,
                    int64_t n_outs, int64_t n_terms, const double* s_table, const char* who)
{
    for (auto& tm : ht)
        if (!CPLX) tm.src_real = tm.s_real = 0;
    for (int64_t i = 0; i < n_outs; ++i) {
        const cyb_tree_from_dense_out& o = outs[i];
        CYB_REQUIRE(o.n_levels >= 0 && o.n_levels <= NK && o.n_k >= 0 && o.n_k <= NK, "%s: output %lld: %d levels and %d contracted levels, at most %d each",
                    who, (long long)i, (int)o.n_levels, (int)o.n_k, NK);
        CYB_REQUIRE_TERM_RANGE(who, i, o, n_terms);
        BwdRec r;
        memset(&r, 0, sizeof(r));
        int64_t total;
        const int64_t* const strides[2] = {o.sd, o.ss};
        for (int l = 0; l < o.n_levels; ++l) CYB_REQUIRE(o.ext[l] >= 0, "%s: output %lld: negative extent", who, (long long)i);
        CYB_REQUIRE(make_levels(r.lv, o.n_levels, o.ext, strides, total), "%s: output %lld: extent too large", who, (long long)i);
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
        for (int j = 0; j < NK; ++j) r.kext[j] = 1;
        int at = NK - o.n_k;
        for (int j = 0; j < o.n_k; ++j, ++at) {
            r.kext[at] = (int32_t)o.kext[j];
            r.kst[at] = o.ks[j];
            r.kwr[at] = -(o.kext[j] - 1) * o.ks[j];
        }
        r.ktotal = (int32_t)ktotal;
        r.divisor = o.divisor;
        r.dst = o.dst, r.first_term = o.first_term, r.n_terms = o.n_terms;
        recs.push_back(r);
        totals.push_back(total);
    }
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
    std::vector<FwdRec> recs;
    std::vector<int64_t> totals;
    CYB_TRY(plan_to_dense<CPLX>(recs, totals, ht, outs, n_outs, n_terms, s_table, who));
    std::vector<FwdItem> items;
    cut_items(items, recs, totals);
    return launch_items(ctx, to_dense_kernel<CPLX>, recs, ht, items, who, s_table);
}

template <bool CPLX>
int tree_from_dense(cyb_ctx_t ctx, const cyb_tree_from_dense_out* outs, int64_t n_outs, const BwdTerm* terms, int64_t n_terms, const double* s_table,
                    const char* who)
{
    CYB_REQUIRE(ctx, "%s: ctx is NULL", who);
    CYB_REQUIRE(n_outs >= 0 && n_terms >= 0 && (n_outs == 0 || outs) && (n_terms == 0 || terms), "%s: bad lists", who);
    if (n_outs == 0) return CYB_OK;
    std::vector<BwdTerm> ht(terms, terms + n_terms);
    std::vector<BwdRec> recs;
    std::vector<int64_t> totals;
    CYB_TRY(plan_from_dense<CPLX>(recs, totals, ht, outs, n_outs, n_terms, s_table, who));
    std::vector<BwdItem> items;
    cut_items(items, recs, totals);
    return launch_items(ctx, from_dense_kernel<CPLX>, recs, ht, items, who, s_table);
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
