// One wave per work item over a mixed-radix index space: the machinery shared by the fusion-tree kernels that write strided
// tiles in ONE launch (tree_outer.hip, tree_compose.hip, tree_dense.hip, tree_place.hip, tree_strip.hip).
//
// A *record* is an index space of up to L levels in C order (the last level fastest) with S offset streams -- destination,
// sources -- that each have a stride per level.  The levels in use are first .. L - 1; the ones before them have extent 1
// and stride 0, so a kernel whose records fill the table from the right may walk all L levels or only the used ones.
//   * host: every record is cut into work items of kMinChunk..kMaxChunk flat units (chunk_for), ONE WAVE owns an item (four
//     items per workgroup, no LDS, no barrier), so that one launch balances thousands of 1 x 1 tiles -- a wave each -- beside
//     a tile of tens of MB.  An item carries the digits and the stream offsets of its first unit (start_at).
//   * device: a lane keeps a cursor (the digits, one running offset per stream).  It decodes its lane offset (below 64:
//     32-bit divisions) once per item (start) and then advances by the wave's step of 64 units with the precomputed digits
//     of the step and a precomputed offset correction per wrap of a level (advance): additions and compares only, no
//     division per element.
//   * item and record are wave-uniform (my_item): their fields travel through scalar loads.
// The tables, the cursor and the host side compile without HIP, so that a plain C++ program can walk them
// (tests/wave_items_walk.cpp).
#pragma once
#ifdef __HIPCC__
#include "flat_items.h"
#define WI_HD __host__ __device__
#else
#define WI_HD
#endif

#include <algorithm>
#include <cstdint>
#include <vector>

namespace cyb_items {

constexpr int NT = 256, WAVE = 64, ITEMS_PER_GROUP = NT / WAVE;
constexpr int64_t kMinChunk = 1024, kMaxChunk = 16384, kTargetItems = 8192; // flat units per work item (multiples of WAVE)

// what a lane holds per step: one double, two adjacent doubles, or one complex number
enum { kF64 = 0, kF64x2 = 1, kC128 = 2 };

inline bool even_(int64_t v) { return (v & 1) == 0; }

// the level table of a record
template <int L, int S> struct Levels {
    int32_t ext[L];
    int32_t step[L];   // digits of the step of WAVE units
    int64_t st[S][L];  // stride of every level in every stream
    int64_t wr[S][L];  // correction of a stream's offset when level l wraps: st[l - 1] - ext[l] * st[l]
    int64_t step_o[S]; // increment of a stream's offset per step, before corrections
    int32_t first, reserved;
};

// digits and stream offsets of one flat unit
template <int L, int S> struct Start {
    int64_t off[S];
    int32_t idx[L];
};

template <int L, int S> struct Item {
    int32_t rec;
    int32_t reserved;
    int64_t count; // flat units of this item
    Start<L, S> at; // its first unit
};

template <int L, int S> struct Cursor {
    int32_t idx[L];
    int64_t off[S];
};

// ---- host: level tables and work items ---------------------------------------------------------------------------------

// Completes a table whose ext[], st[][] of the levels first .. L - 1 are set: the wrap corrections and the digits of the step.
// What is left of the step at the outermost used level stays there (a cursor is only read while inside the record).
template <int L, int S> void set_steps(Levels<L, S>& t, int first)
{
    t.first = first;
    for (int l = 0; l < first; ++l) {
        t.ext[l] = 1, t.step[l] = 0;
        for (int a = 0; a < S; ++a) t.st[a][l] = t.wr[a][l] = 0;
    }
    for (int a = 0; a < S; ++a) t.step_o[a] = 0;
    int64_t s = WAVE;
    for (int l = L - 1; l >= first; --l) {
        for (int a = 0; a < S; ++a) t.wr[a][l] = (l > first ? t.st[a][l - 1] : 0) - t.ext[l] * t.st[a][l];
        t.step[l] = (int32_t)(l > first ? s % t.ext[l] : std::min<int64_t>(s, t.ext[l]));
        s = l > first ? s / t.ext[l] : 0;
        for (int a = 0; a < S; ++a) t.step_o[a] += t.step[l] * t.st[a][l];
    }
}

// the product of `n` extents if it equals `want`; extents are within [0, 2^30], want is at most 2^60
inline bool product_is(const int64_t* ext, int n, int64_t want)
{
    for (int l = 0; l < n; ++l)
        if (ext[l] == 0) return want == 0;
    int64_t p = 1;
    for (int l = 0; l < n; ++l) {
        p *= ext[l];
        if (p > ((int64_t)1 << 61)) return false;
    }
    return p == want;
}

// The levels (ext[l], st[l]), l < n in C order, of a strided view that is walked in C order, in place: a level of extent 1 is
// dropped and a level that continues its inner neighbour is merged into it while the extent stays within max_extent (a
// contiguous tile of a block: one row level, one column level).  Returns the number of levels left.
inline int merge_levels(int64_t* ext, int64_t* st, int n, int64_t max_extent)
{
    int m = 0; // levels kept so far, the innermost first
    for (int l = n - 1; l >= 0; --l) {
        if (ext[l] == 1) continue;
        if (m > 0 && (__int128)st[l] == (__int128)ext[n - m] * st[n - m] && ext[l] * ext[n - m] <= max_extent)
            ext[n - m] *= ext[l];
        else
            ++m, ext[n - m] = ext[l], st[n - m] = st[l];
    }
    for (int l = 0; l < m; ++l) ext[l] = ext[n - m + l], st[l] = st[n - m + l];
    return m;
}

// flat units per work item: about kTargetItems waves for a large launch
inline int64_t chunk_for(const std::vector<int64_t>& totals)
{
    int64_t grand = 0;
    for (int64_t t : totals) grand += t;
    const int64_t chunk = (grand / kTargetItems + WAVE - 1) / WAVE * WAVE;
    return std::min(std::max(chunk, kMinChunk), kMaxChunk);
}

// digits and stream offsets of the flat unit e
template <int L, int S> Start<L, S> start_at(const Levels<L, S>& t, int64_t e)
{
    Start<L, S> s = {};
    for (int l = L - 1; l >= t.first; --l) {
        s.idx[l] = (int32_t)(e % t.ext[l]);
        e /= t.ext[l];
        for (int a = 0; a < S; ++a) s.off[a] += s.idx[l] * t.st[a][l];
    }
    return s;
}

// cuts record i of totals[i] flat units, whose level table is recs[i].lv, into items
template <class RecT, int L, int S> void cut_items(std::vector<Item<L, S>>& items, const std::vector<RecT>& recs, const std::vector<int64_t>& totals)
{
    const int64_t chunk = chunk_for(totals);
    for (size_t i = 0; i < recs.size(); ++i)
        for (int64_t e0 = 0; e0 < totals[i]; e0 += chunk)
            items.push_back(Item<L, S>{(int32_t)i, 0, std::min(chunk, totals[i] - e0), start_at(recs[i].lv, e0)});
}

// ---- the cursor --------------------------------------------------------------------------------------------------------

// c += (digits dg, whose stream offsets are d) over the levels first .. L - 1; every digit below its extent, so a level wraps
// at most once
template <int L, int S>
WI_HD inline void advance(Cursor<L, S>& c, const Levels<L, S>& t, const int32_t (&dg)[L], const int64_t (&d)[S], int first)
{
#pragma unroll
    for (int a = 0; a < S; ++a) c.off[a] += d[a];
    int32_t carry = 0;
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
        if (l >= first) { // wave-uniform
            const int32_t i = c.idx[l] + dg[l] + carry;
            const bool w = i >= t.ext[l];
            c.idx[l] = w ? i - t.ext[l] : i;
#pragma unroll
            for (int a = 0; a < S; ++a) c.off[a] += w ? t.wr[a][l] : 0;
            carry = w ? 1 : 0;
        }
    }
}

// the cursor of `lane` at the start of an item
template <int L, int S> WI_HD inline void start(Cursor<L, S>& c, const Levels<L, S>& t, const Start<L, S>& at, int lane, int first)
{
#pragma unroll
    for (int l = 0; l < L; ++l) c.idx[l] = at.idx[l];
#pragma unroll
    for (int a = 0; a < S; ++a) c.off[a] = at.off[a];
    // lane offset into the item -> digits (below 64: 32-bit divisions, extents above it never divide)
    uint32_t d = (uint32_t)lane;
    int32_t dg[L];
    int64_t dd[S];
#pragma unroll
    for (int a = 0; a < S; ++a) dd[a] = 0;
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
        dg[l] = 0;
        if (l < first) continue;
        const uint32_t e32 = t.ext[l] > WAVE ? (uint32_t)WAVE + 1 : (uint32_t)t.ext[l];
        const uint32_t q = d / e32;
        dg[l] = (int32_t)(d - q * e32);
        d = q;
#pragma unroll
        for (int a = 0; a < S; ++a) dd[a] += dg[l] * t.st[a][l];
    }
    advance(c, t, dg, dd, first);
}

#ifdef __HIPCC__
// ---- device: the kernel prologue, loads and stores ---------------------------------------------------------------------

// one wave per item: the index is wave-uniform, and so is everything read through it.  false: no item for this wave
__device__ inline bool my_item(int& i, int& lane, int n_items)
{
    i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ITEMS_PER_GROUP + threadIdx.x / WAVE));
    lane = threadIdx.x & (WAVE - 1);
    return i < n_items;
}

template <int MODE> struct Val { typedef d2 type; };
template <> struct Val<kF64> { typedef double type; };

template <int MODE> __device__ inline typename Val<MODE>::type zero_()
{
    if constexpr (MODE == kF64) return 0.0; else return d2{0.0, 0.0};
}

// offsets in doubles; kC128: in complex elements
template <int MODE> __device__ inline void store_(double* dst_, int64_t o, typename Val<MODE>::type v)
{
    GLOBAL_AS double* dst = (GLOBAL_AS double*)dst_;
    if constexpr (MODE == kF64)
        dst[o] = v;
    else if constexpr (MODE == kF64x2)
        *(GLOBAL_AS d2*)(dst + o) = v;
    else
        *(GLOBAL_AS d2*)(dst + 2 * o) = v;
}

__device__ inline double load_f64(const double* p, int64_t o) { return ((const GLOBAL_AS double*)p)[o]; }

// two adjacent doubles in one 16-byte load
__device__ inline d2 load_x2(const double* p, int64_t o) { return *(const GLOBAL_AS d2*)((const GLOBAL_AS double*)p + o); }

// a value of `p` at element offset o: complex storage, or float64 storage read as it stands
__device__ inline d2 load_c(const double* p_, int64_t o, bool real)
{
    const GLOBAL_AS double* p = (const GLOBAL_AS double*)p_;
    return real ? d2{p[o], 0.0} : *(const GLOBAL_AS d2*)(p + 2 * o);
}

// ---- host: the term range of an output, the launch of a kernel (recs, terms, items, n_items, extra...) -----------------

#define CYB_REQUIRE_TERM_RANGE(who, i, o, n_terms)                                                                                        \
    CYB_REQUIRE((o).first_term >= 0 && (o).n_terms >= 0 && (o).first_term <= (n_terms) && (o).n_terms <= (n_terms) - (o).first_term,       \
                "%s: output %lld: bad term range [%lld, +%lld)", who, (long long)(i), (long long)(o).first_term, (long long)(o).n_terms)

// the launch tail of flat_items.h with four items per workgroup; the kernel learns the number of items
template <class RecT, class TermT, class ItemT, class... Extra>
int launch_items(cyb_ctx_t ctx, void (*kernel)(const RecT*, const TermT*, const ItemT*, int, Extra...), const std::vector<RecT>& recs,
                 const std::vector<TermT>& terms, const std::vector<ItemT>& items, const char* who, Extra... extra)
{
    return cyb_flat::launch<ITEMS_PER_GROUP>(ctx, who, kernel, cyb_flat::arrays(recs, terms, items), (int)items.size(), extra...);
}
#endif // __HIPCC__

} // namespace cyb_items
