// Strided N-d copies: the device bodies and the host-side classification shared by the batched copy of blockops.hip
// (descriptors with addresses, built per call) and the placement plans of place_plan.hip (records with block numbers,
// built once; the addresses come from two tables at enqueue time).  The work item of a body is the flat Item of
// flat_items.h: a range of elements (strided body) or of tiles (transposing bodies).
#pragma once
#include "flat_items.h"

namespace cyb_copy {

using cyb_flat::Item;
using cyb_flat::NT;

// ---------------------------------------------------------------------------------------------
// strided copy
struct CopyDev {
    void* dst;
    const void* src;
    int32_t ndim, conj;
    int64_t total;
    int64_t shape[CYB_MAX_NDIM];
    int64_t ds[CYB_MAX_NDIM];
    int64_t ss[CYB_MAX_NDIM];
};

typedef unsigned long long u128 __attribute__((ext_vector_type(2)));

// One wave copies one contiguous run of n elements: 16-byte accesses when source and destination are misaligned the
// same way (one element peeled), four independent accesses in flight per lane.
template <typename V>
__device__ __forceinline__ void wave_copy_run(const GLOBAL_AS V* sp, GLOBAL_AS V* dp, int64_t n, int lane, int W = 64)
{
    int64_t i = lane;
    for (; i + 3 * W < n; i += 4 * W) {
        const V a = sp[i], b = sp[i + W], c = sp[i + 2 * W], e = sp[i + 3 * W];
        dp[i] = a;
        dp[i + W] = b;
        dp[i + 2 * W] = c;
        dp[i + 3 * W] = e;
    }
    for (; i < n; i += W) dp[i] = sp[i];
}
// W = 64: the calling wave owns the run; W = NT: the whole workgroup shares it (lane = threadIdx.x)
__device__ __forceinline__ void wave_copy_row8(const GLOBAL_AS uint64_t* sp, GLOBAL_AS uint64_t* dp, int64_t n, int lane, int W = 64)
{
    if (n <= 0) return;
    const unsigned ms = (unsigned)((uintptr_t)sp & 15), md = (unsigned)((uintptr_t)dp & 15);
    if (ms != md) {
        wave_copy_run<uint64_t>(sp, dp, n, lane, W);
        return;
    }
    if (ms) {
        if (lane == 0) dp[0] = sp[0];
        ++sp, ++dp, --n;
    }
    wave_copy_run<u128>((const GLOBAL_AS u128*)sp, (GLOBAL_AS u128*)dp, n >> 1, lane, W);
    if ((n & 1) && lane == 0) dp[n - 1] = sp[n - 1];
}

// work item `it` of the copy `d` from `src` to `dst` (the addresses of d itself are not read)
template <typename T>
__device__ __forceinline__ void copy_strided_body(const CopyDev& d, const GLOBAL_AS T* src, GLOBAL_AS T* dst, const Item& it)
{
    // The innermost (merged) axis is contiguous on both sides in most copies (plain copies, the sub-block scatter of
    // combine_legs, the gather of split_legs, permutations that keep the last axis): every wave walks whole rows of it
    // -- no division per element, the outer index is decoded once per row, 16-byte accesses where the alignment allows.
    const int last = d.ndim - 1;
    if (d.ndim >= 1 && d.ss[last] == 1 && d.ds[last] == 1 && d.shape[last] >= 16 && !(sizeof(T) == 16 && d.conj)) {
        const int64_t inner = d.shape[last];
        const int64_t e0 = it.start, e1 = it.start + it.count;
        const int64_t r0 = e0 / inner, r1 = (e1 - 1) / inner;
        // short rows: one wave per row (four rows in flight per workgroup); long rows: the waves share a row
        const bool shared_row = inner >= 2048;
        const int wave = shared_row ? 0 : (int)(threadIdx.x >> 6), lane = shared_row ? (int)threadIdx.x : (int)(threadIdx.x & 63);
        for (int64_t row = r0 + wave; row <= r1; row += shared_row ? 1 : NT / 64) {
            const int64_t c0 = (row == r0) ? e0 - r0 * inner : 0;
            const int64_t c1 = (row == r1) ? e1 - r1 * inner : inner;
            int64_t rem = row, so = 0, dof = 0;
            for (int k = last - 1; k >= 0; --k) {
                const int64_t sh = d.shape[k];
                const int64_t q = rem / sh, i = rem - q * sh;
                rem = q;
                so += i * d.ss[k];
                dof += i * d.ds[k];
            }
            const GLOBAL_AS T* sp = src + so + c0;
            GLOBAL_AS T* dp = dst + dof + c0;
            const int W = shared_row ? NT : 64;
            if constexpr (sizeof(T) == 8) wave_copy_row8((const GLOBAL_AS uint64_t*)sp, (GLOBAL_AS uint64_t*)dp, c1 - c0, lane, W);
            else wave_copy_run<T>(sp, dp, c1 - c0, lane, W);
        }
        return;
    }
    for (int64_t e = it.start + threadIdx.x; e < it.start + it.count; e += NT) {
        int64_t rem = e, so = 0, dof = 0;
#pragma unroll
        for (int k = CYB_MAX_NDIM - 1; k >= 0; --k) {
            if (k < d.ndim) {
                const int64_t sh = d.shape[k];
                const int64_t q = rem / sh, i = rem - q * sh;
                rem = q;
                so += i * d.ss[k];
                dof += i * d.ds[k];
            }
        }
        T v = src[so];
        if constexpr (sizeof(T) == 16) {
            if (d.conj) v.y ^= 0x8000000000000000ull; // flip the sign of the imaginary part
        }
        dst[dof] = v;
    }
}


// Transposing copies (the fastest axis of the destination is not the fastest axis of the source: permute_axes
// of a compose operand, the leg rotations of a Krylov matvec): 32 x 32 tiles through LDS so that BOTH the reads
// (along the source's unit-stride axis S) and the writes (along the destination's unit-stride axis D) are
// coalesced, and the index arithmetic (64-bit div/mod over up to 8 axes) runs once per tile, not per element.
struct CopyT {
    void* dst;
    const void* src;
    int32_t n_outer, conj;
    int64_t nS, nD;       // extents of the two tiled axes
    int64_t ssD, dsS;     // source stride of D, destination stride of S (ss of S and ds of D are 1)
    // A tiled axis may be the flattening of TWO axes that are contiguous on its own side (a short innermost axis
    // such as the MPO bond of [.., vR, wR] and its neighbour): index i of D then sits at source offset
    // (i / nD2) * ssD + (i % nD2) * ssD2, index i of S at destination offset (i / nS2) * dsS + (i % nS2) * dsS2.
    // nD2 = nS2 = 1 for a plain axis.
    int64_t nD2, ssD2, nS2, dsS2;
    int64_t tilesS, tilesD;
    int64_t oshape[CYB_MAX_NDIM], ods[CYB_MAX_NDIM], oss[CYB_MAX_NDIM]; // the remaining (outer) axes
};

// `tile`: the workgroup's LDS image, T[32][33]
template <typename T>
__device__ __forceinline__ void copy_transpose_body(const CopyT& d, const GLOBAL_AS T* src, GLOBAL_AS T* dst, const Item& it, T (*tile)[33])
{
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int64_t t = it.start; t < it.start + it.count; ++t) {
        int64_t rem = t;
        const int64_t td = rem % d.tilesD;
        rem /= d.tilesD;
        const int64_t ts = rem % d.tilesS;
        rem /= d.tilesS;
        int64_t so = 0, dof = 0;
        for (int k = d.n_outer - 1; k >= 0; --k) {
            const int64_t q = rem / d.oshape[k], i = rem - q * d.oshape[k];
            rem = q;
            so += i * d.oss[k];
            dof += i * d.ods[k];
        }
        const int64_t s0 = ts * 32, d0 = td * 32;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t sI = s0 + tx, dI = d0 + ty + 8 * q;
            if (sI < d.nS && dI < d.nD) {
                T v = src[so + sI + (dI / d.nD2) * d.ssD + (dI % d.nD2) * d.ssD2];
                if constexpr (sizeof(T) == 16) {
                    if (d.conj) v.y ^= 0x8000000000000000ull;
                }
                tile[ty + 8 * q][tx] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t dI = d0 + tx, sI = s0 + ty + 8 * q;
            if (sI < d.nS && dI < d.nD) dst[dof + dI + (sI / d.nS2) * d.dsS + (sI % d.nS2) * d.dsS2] = tile[tx][ty + 8 * q];
        }
        __syncthreads();
    }
}

// 8-byte elements: 64 x 64 tiles, two elements per 16-byte access on both sides (falls back to 8-byte accesses
// row by row when a row start is not 16-byte aligned).  LDS image is [s][d] so that the write phase reads pairs.
constexpr int T64_TS = 64, T64_LS = T64_TS + 2; // `tile` of the body below: double[T64_TS * T64_LS], 16-byte aligned
__device__ __forceinline__ void copy_transpose64_body(const CopyT& d, gcp src, gp dst, const Item& it, double* tile)
{
    constexpr int TS = T64_TS, LS = T64_LS; // tile[s * LS + d]
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int64_t t = it.start; t < it.start + it.count; ++t) {
        int64_t rem = t;
        const int64_t td = rem % d.tilesD;
        rem /= d.tilesD;
        const int64_t ts = rem % d.tilesS;
        rem /= d.tilesS;
        int64_t so = 0, dof = 0;
        for (int k = d.n_outer - 1; k >= 0; --k) {
            const int64_t q = rem / d.oshape[k], i = rem - q * d.oshape[k];
            rem = q;
            so += i * d.oss[k];
            dof += i * d.ods[k];
        }
        const int64_t s0 = ts * TS, d0 = td * TS;
#pragma unroll
        for (int q = 0; q < 8; ++q) { // read: rows along D, pairs along S
            const int64_t dI = d0 + ty + 8 * q, sI = s0 + 2 * tx;
            if (dI < d.nD && sI < d.nS) {
                gcp p = src + so + (dI / d.nD2) * d.ssD + (dI % d.nD2) * d.ssD2 + sI;
                double v0, v1 = 0.0;
                if (sI + 1 < d.nS && (((uintptr_t)p) & 15) == 0) {
                    const d2 v = *(const GLOBAL_AS d2*)p;
                    v0 = v.x;
                    v1 = v.y;
                } else {
                    v0 = p[0];
                    if (sI + 1 < d.nS) v1 = p[1];
                }
                tile[(2 * tx) * LS + ty + 8 * q] = v0;
                tile[(2 * tx + 1) * LS + ty + 8 * q] = v1;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) { // write: rows along S, pairs along D
            const int64_t sI = s0 + ty + 8 * q, dI = d0 + 2 * tx;
            if (sI < d.nS && dI < d.nD) {
                gp p = dst + dof + (sI / d.nS2) * d.dsS + (sI % d.nS2) * d.dsS2 + dI;
                const d2 v = *reinterpret_cast<const d2*>(&tile[(ty + 8 * q) * LS + 2 * tx]);
                if (dI + 1 < d.nD && (((uintptr_t)p) & 15) == 0) {
                    *(GLOBAL_AS d2*)p = v;
                } else {
                    p[0] = v.x;
                    if (dI + 1 < d.nD) p[1] = v.y;
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// host side: what one copy becomes

// `c` := the copy (shape, dst_strides, src_strides) with its singleton axes dropped and the axes that are contiguous in
// BOTH operands merged; c.total = number of elements.  false: a negative extent.
inline bool normalize_copy(const int64_t* shape, const int64_t* dst_strides, const int64_t* src_strides, int ndim, CopyDev& c)
{
    int64_t tot = 1;
    int nd = 0;
    for (int k = 0; k < ndim; ++k) {
        if (shape[k] < 0) return false;
        tot *= shape[k];
        if (shape[k] == 1) continue;
        if (nd > 0 && c.ds[nd - 1] == dst_strides[k] * shape[k] && c.ss[nd - 1] == src_strides[k] * shape[k]) {
            c.shape[nd - 1] *= shape[k];
            c.ds[nd - 1] = dst_strides[k];
            c.ss[nd - 1] = src_strides[k];
        } else {
            c.shape[nd] = shape[k];
            c.ds[nd] = dst_strides[k];
            c.ss[nd] = src_strides[k];
            ++nd;
        }
    }
    for (int k = nd; k < CYB_MAX_NDIM; ++k) {
        c.shape[k] = 1;
        c.ds[k] = c.ss[k] = 0;
    }
    c.ndim = nd;
    c.total = tot;
    return true;
}

// Transposing copy?  (unit-stride axes of source and destination differ and are both long enough.)  true: `t` holds the
// tiled form of the normalized copy `c` (addresses and conj left zero) for tiles of `tsz` x `tsz`, `ntile` their number.
inline bool classify_transpose(const CopyDev& c, int64_t tsz, CopyT& t, int64_t& ntile)
{
    const int nd = c.ndim;
    int aS = -1, aD = -1;
    for (int k = 0; k < nd; ++k) {
        if (c.ss[k] == 1 && aS < 0) aS = k;
        if (c.ds[k] == 1 && aD < 0) aD = k;
    }
    // a short unit-stride axis may be flattened with the axis that is next-contiguous on the same side
    int pD = -1, pS = -1; // partner axes (outer halves of the composites)
    if (aS >= 0 && aD >= 0 && aS != aD) {
        if (c.shape[aD] < 16)
            for (int k = 0; k < nd; ++k)
                if (k != aD && k != aS && c.ds[k] == c.shape[aD]) pD = k;
        if (c.shape[aS] < 16)
            for (int k = 0; k < nd; ++k)
                if (k != aS && k != aD && k != pD && c.ss[k] == c.shape[aS]) pS = k;
    }
    const int64_t extS = aS >= 0 ? c.shape[aS] * (pS >= 0 ? c.shape[pS] : 1) : 0;
    const int64_t extD = aD >= 0 ? c.shape[aD] * (pD >= 0 ? c.shape[pD] : 1) : 0;
    if (!(c.total > 0 && aS >= 0 && aD >= 0 && aS != aD && extS >= 16 && extD >= 16)) return false;
    memset(&t, 0, sizeof(t));
    t.nS = extS;
    t.nD = extD;
    if (pD >= 0) {
        t.nD2 = c.shape[aD];
        t.ssD = c.ss[pD];
        t.ssD2 = c.ss[aD];
    } else {
        t.nD2 = 1;
        t.ssD = c.ss[aD];
        t.ssD2 = 0;
    }
    if (pS >= 0) {
        t.nS2 = c.shape[aS];
        t.dsS = c.ds[pS];
        t.dsS2 = c.ds[aS];
    } else {
        t.nS2 = 1;
        t.dsS = c.ds[aS];
        t.dsS2 = 0;
    }
    t.tilesS = (t.nS + tsz - 1) / tsz;
    t.tilesD = (t.nD + tsz - 1) / tsz;
    int64_t outer = 1;
    for (int k = 0; k < nd; ++k) {
        if (k == aS || k == aD || k == pS || k == pD) continue;
        t.oshape[t.n_outer] = c.shape[k];
        t.ods[t.n_outer] = c.ds[k];
        t.oss[t.n_outer] = c.ss[k];
        ++t.n_outer;
        outer *= c.shape[k];
    }
    ntile = outer * t.tilesS * t.tilesD;
    return true;
}
// tiles per work item of the transposing kernels
inline int64_t tiles_per_item(int64_t tsz) { return tsz == 64 ? 4 : 16; }

} // namespace cyb_copy
