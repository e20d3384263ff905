// HBM-bound block-list operations (gfx950): strided N-d copies, BLAS-1 reductions and
// elementwise ops, axis scaling, mask gather/scatter, fills, RNG.
//
// These replace the numpy calls behind the data-movement and BLAS-1 virtuals of the reference's
// NumpyBlockBackend (src/block_backend/numpy.cpp: permute_axes :924-931, reshape :1057-1064,
// apply_mask :605-613, enlarge_leg :700-728, scale_axis :1373-1385, norm :898-913, inner :815-842,
// linear_combination :1358-1365, eye_matrix :1197-1207, zeros :1322-1335) -- one launch per block
// LIST instead of one numpy call per block.  All are bandwidth-class work: 16-B accesses where
// the layout allows, grid-stride loops, deterministic two-stage reductions (no float atomics).
// Work items, their cutter, the launch tail and the fixed order of the reductions: flat_items.h.
#include "common.h"
#include "copy_kernels.h"

#include <algorithm>
#include <type_traits>

namespace {

using namespace cyb_copy; // the copy descriptors and device bodies
using namespace cyb_flat; // Item, NT, the chunk rules, cut, launch, the fixed-order reduction

// ---------------------------------------------------------------------------------------------
// strided copy (device bodies: copy_kernels.h)
template <typename T>
__global__ void __launch_bounds__(NT) copy_strided_kernel(const CopyDev* __restrict__ descs, const Item* __restrict__ items)
{
    const Item it = items[blockIdx.x];
    const CopyDev d = descs[it.desc];
    copy_strided_body<T>(d, (const GLOBAL_AS T*)d.src, (GLOBAL_AS T*)d.dst, it);
}

template <typename T>
__global__ void __launch_bounds__(NT) copy_transpose_kernel(const CopyT* __restrict__ descs, const Item* __restrict__ items)
{
    __shared__ T tile[32][33];
    const Item it = items[blockIdx.x];
    const CopyT d = descs[it.desc];
    copy_transpose_body<T>(d, (const GLOBAL_AS T*)d.src, (GLOBAL_AS T*)d.dst, it, tile);
}

__global__ void __launch_bounds__(NT) copy_transpose64_kernel(const CopyT* __restrict__ descs, const Item* __restrict__ items)
{
    __shared__ __attribute__((aligned(16))) double tile[T64_TS * T64_LS];
    const Item it = items[blockIdx.x];
    const CopyT d = descs[it.desc];
    copy_transpose64_body(d, (gcp)d.src, (gp)d.dst, it, tile);
}


// ---------------------------------------------------------------------------------------------
// complex128 support of the tdot path.  A complex block is stored interleaved (re, im) like numpy's
// complex128.  A complex product C = A B runs through the SAME real f64-MFMA grouped GEMM: A (M x K complex,
// k-contiguous) is read in place as the real M x 2K matrix [ar0 ai0 ar1 ai1 ...], C (M x N complex) is written in
// place as the real M x 2N matrix, and B is expanded once into the real 2K x 2N matrix
//        B'[2k][2n] = br   B'[2k][2n+1] = bi   B'[2k+1][2n] = -bi   B'[2k+1][2n+1] = br
// so that A_real B' = C_real.  8 M N K real flops -- exactly the four real products of a complex one.
struct CExpandDev {
    const double* src; // complex elements (re, im)
    int64_t rs, cs;    // strides of src in complex elements
    int64_t K, N;
    double* dst;       // 2K x 2N doubles, row-major, contiguous
};

__global__ void __launch_bounds__(NT) complex_expand_kernel(const CExpandDev* __restrict__ descs, const Item* __restrict__ items)
{
    const Item it = items[blockIdx.x];
    const CExpandDev d = descs[it.desc];
    const GLOBAL_AS d2* src = (const GLOBAL_AS d2*)d.src;
    gp dst = (gp)d.dst;
    for (int64_t e = it.start + threadIdx.x; e < it.start + it.count; e += NT) {
        const int64_t k = e / d.N, n = e - k * d.N;
        const d2 b = src[k * d.rs + n * d.cs];
        GLOBAL_AS d2* r0 = (GLOBAL_AS d2*)(dst + (2 * k) * (2 * d.N) + 2 * n);
        GLOBAL_AS d2* r1 = (GLOBAL_AS d2*)(dst + (2 * k + 1) * (2 * d.N) + 2 * n);
        *r0 = d2{b.x, b.y};
        *r1 = d2{-b.y, b.x};
    }
}

// ---------------------------------------------------------------------------------------------
// reductions (two-stage, deterministic)
struct VecDev {
    const double* x;
    const double* y;
    double* out;
    int64_t n;
};

// partial[item] of Op = Sum: sum x*y (y null: x*x) ; Op = NanMax: max |x|, NaN if any element is NaN
template <class Op> __device__ __forceinline__ void reduce_stage1_body(const VecDev& d, const Item& it, double* __restrict__ partial)
{
    __shared__ double red[1][WAVES];
    gcp x = (gcp)d.x;
    gcp y = (gcp)d.y;
    double acc = 0.0;
    const int64_t e1 = it.start + it.count;
    // 16-byte accesses when the operands allow (chunk starts are even): half the memory instructions per byte
    const bool al = ((((uintptr_t)(x + it.start)) | (d.y ? (uintptr_t)(y + it.start) : 0)) & 15) == 0;
    const int64_t nv = al ? it.count / 2 : 0;
    const GLOBAL_AS d2* xv = (const GLOBAL_AS d2*)(x + it.start);
    const GLOBAL_AS d2* yv = (const GLOBAL_AS d2*)(y + it.start);
    if constexpr (std::is_same<Op, Sum>::value) {
        double acc2 = 0.0;
        if (d.y) {
            for (int64_t i = threadIdx.x; i < nv; i += NT) {
                const d2 a = xv[i], b = yv[i];
                acc += a.x * b.x;
                acc2 += a.y * b.y;
            }
            for (int64_t e = it.start + 2 * nv + threadIdx.x; e < e1; e += NT) acc += x[e] * y[e];
        } else {
            for (int64_t i = threadIdx.x; i < nv; i += NT) {
                const d2 a = xv[i];
                acc += a.x * a.x;
                acc2 += a.y * a.y;
            }
            for (int64_t e = it.start + 2 * nv + threadIdx.x; e < e1; e += NT) acc += x[e] * x[e];
        }
        acc += acc2;
    } else {
        for (int64_t i = threadIdx.x; i < nv; i += NT) {
            const d2 a = xv[i];
            acc = Op::op(acc, Op::op(fabs(a.x), fabs(a.y)));
        }
        for (int64_t e = it.start + 2 * nv + threadIdx.x; e < e1; e += NT) acc = Op::op(acc, fabs(x[e]));
    }
    double r[1] = {acc};
    block_reduce<1, Op>(r, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = r[0];
}
template <class Op>
__global__ void __launch_bounds__(NT) reduce_stage1_kernel(const VecDev* __restrict__ descs, const Item* __restrict__ items, double* __restrict__ partial)
{
    const Item it = items[blockIdx.x];
    const VecDev d = descs[it.desc];
    reduce_stage1_body<Op>(d, it, partial);
}
// ONE vector: descriptor and chunking travel as kernel arguments -- no descriptor upload (a host call and a copy kernel per
// launch: most BLAS-1 calls of a Krylov iteration on flat pools are of this kind)
template <class Op> __global__ void __launch_bounds__(NT) reduce_stage1_one_kernel(VecDev d, int64_t chunk, double* __restrict__ partial)
{
    reduce_stage1_body<Op>(d, nth_item(chunk, d.n), partial);
}

// out = a*x + b*y on complex vectors (a, b complex scalars; y may be null)
__global__ void __launch_bounds__(NT) axpby_c128_kernel(const VecDev* __restrict__ descs, const Item* __restrict__ items,
                                                        double ar, double ai, double br, double bi)
{
    const Item it = items[blockIdx.x];
    const VecDev d = descs[it.desc];
    const GLOBAL_AS d2* x = (const GLOBAL_AS d2*)d.x;
    const GLOBAL_AS d2* y = (const GLOBAL_AS d2*)d.y;
    GLOBAL_AS d2* out = (GLOBAL_AS d2*)d.out;
    for (int64_t e = it.start + threadIdx.x; e < it.start + it.count; e += NT) {
        const d2 xv = x[e];
        d2 r = d2{ar * xv.x - ai * xv.y, ar * xv.y + ai * xv.x};
        if (d.y) {
            const d2 yv = y[e];
            r.x += br * yv.x - bi * yv.y;
            r.y += br * yv.y + bi * yv.x;
        }
        out[e] = r;
    }
}

// complex elementwise: op 0 |z| (real out), 1 sqrt, 2 exp, 3 log, 4 angle (real out), 5 z*w, 6 z/w (Smith).
// Non-finite arguments, signed zeros and arguments near the ends of the double range follow numpy (C99 Annex G):
// tests/special_value_cases.py holds the grid.
typedef d2 cd2;
#define CYB_DBL_MAX 1.7976931348623157e308

// a product rounded on its own: the empty asm keeps -ffp-contract=fast from fusing it into the add that follows
__device__ __forceinline__ double mul_rn(double a, double b)
{
    double p = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(p));
#endif
    return p;
}

// principal square root.  sqrt((|z| + |x|) / 2) with the operands scaled by a power of four where |z| + |x| would overflow
// (1.5e308 + 1e308 i) or where the parts are denormal (the quotient y / 2t would lose its bits)
__device__ __forceinline__ cd2 csqrt_c128(cd2 z)
{
    double x = z.x, y = z.y;
    if (x == 0.0 && y == 0.0) return cd2{0.0, y};
    if (fabs(y) == INFINITY) return cd2{INFINITY, y};          // also for a NaN real part
    if (x != x) return cd2{x, __builtin_nan("")};
    if (fabs(x) == INFINITY) {
        if (x > 0.0) return cd2{x, y != y ? y : copysign(0.0, y)};
        return cd2{y != y ? y : 0.0, copysign(INFINITY, y)};
    }
    if (y != y) return cd2{y, y};
    const double hi = fmax(fabs(x), fabs(y));
    double back = 1.0;
    if (hi > 4e307) {
        x *= 0.25, y *= 0.25, back = 2.0;
    } else if (hi < 1e-290) {
        x *= 0x1p108, y *= 0x1p108, back = 0x1p-54;
    }
    const double t = sqrt(0.5 * (hypot(x, y) + fabs(x)));
    const cd2 r = x >= 0.0 ? cd2{t, y / (2.0 * t)} : cd2{fabs(y) / (2.0 * t), copysign(t, y)};
    return cd2{r.x * back, r.y * back};
}

// sin and cos of an argument of 2^30 and beyond.  The device library's reduction for such arguments came out wrong by about
// |x| 2^-55 on the MI355X (sincos(1.5e12) off by 3e-5, measured against mpmath; below 2^30 it is accurate), so exp of a complex
// number with a large imaginary part reduces the argument itself: Payne-Hanek in integer arithmetic -- the 192 bits of 2 / pi
// that decide the quadrant and the fraction of |x| = m 2^e, times the 53-bit integer m.  64 zero bits (the integer part), then
// the first 1344 bits of 2 / pi:
__device__ const unsigned long long kTwoOverPi[22] = {
    0x0000000000000000ull, 0xa2f9836e4e441529ull, 0xfc2757d1f534ddc0ull, 0xdb6295993c439041ull,
    0xfe5163abdebbc561ull, 0xb7246e3a424dd2e0ull, 0x06492eea09d1921cull, 0xfe1deb1cb129a73eull,
    0xe88235f52ebb4484ull, 0xe99c7026b45f7e41ull, 0x3991d639835339f4ull, 0x9c845f8bbdf9283bull,
    0x1ff897ffde05980full, 0xef2f118b5a0a6d1full, 0x6d367ecf27cb09b7ull, 0x4f463f669e5fea2dull,
    0x7527bac7ebe5f17bull, 0x3d0739f78a5292eaull, 0x6bfb5fb11f8d5d08ull, 0x56033046fc7b6babull,
    0xf0cfbc209af4361dull, 0xa9e391615ee61b08ull
};
__device__ __forceinline__ void sincos_large(double x, double* sn, double* cs)
{
    int E;
    const double fr = frexp(fabs(x), &E);                       // |x| = fr 2^E = m 2^e, m a 53-bit integer
    const unsigned long long m = (unsigned long long)ldexp(fr, 53);
    const int i0 = 62 + (E - 53);                               // first bit of 2/pi (after 64 zero integer bits) whose product with m is below 4
    const int wi = i0 >> 6, bo = i0 & 63;
    unsigned long long v[3];
    for (int k = 0; k < 3; ++k)
        v[k] = bo ? (kTwoOverPi[wi + k] << bo) | (kTwoOverPi[wi + k + 1] >> (64 - bo)) : kTwoOverPi[wi + k];
    // m * (v[0] : v[1] : v[2]) as four 64-bit limbs r3 : r2 : r1 : r0; bit 190 has weight one quadrant
    const unsigned __int128 p0 = (unsigned __int128)m * v[2];
    const unsigned __int128 p1 = (unsigned __int128)m * v[1] + (unsigned long long)(p0 >> 64);
    const unsigned __int128 p2 = (unsigned __int128)m * v[0] + (unsigned long long)(p1 >> 64);
    const unsigned long long r0 = (unsigned long long)p0, r1 = (unsigned long long)p1, r2 = (unsigned long long)p2;
    int q = (int)(r2 >> 62) & 3;
    unsigned long long fh = (r2 << 2) | (r1 >> 62), fl = (r1 << 2) | (r0 >> 62); // the fraction of a quadrant, 128 bits
    double sign = 1.0;
    if (fh >> 63) { // beyond half a quadrant: the next one, from above
        q = (q + 1) & 3;
        fl = ~fl + 1ull;
        fh = ~fh + (fl == 0ull ? 1ull : 0ull);
        sign = -1.0;
    }
    int lz = 0;
    if (fh == 0ull) {
        fh = fl;
        fl = 0ull;
        lz = 64;
    }
    if (fh != 0ull) {
        const int z = __builtin_clzll(fh);
        if (z) fh = (fh << z) | (fl >> (64 - z));
        lz += z;
    }
    // fraction = fh 2^-(64 + lz): its upper 53 bits and the 11 below them, times pi / 2 = hi + lo
    const double f1 = ldexp((double)(fh & ~0x7FFull), -(64 + lz)), f2 = ldexp((double)(fh & 0x7FFull), -(64 + lz));
    const double pio2_hi = 1.5707963267948966, pio2_lo = 6.123233995736766e-17;
    const double rh = f1 * pio2_hi;
    const double r = sign * (rh + (fma(f1, pio2_hi, -rh) + (f1 * pio2_lo + f2 * pio2_hi)));
    double s, c;
    sincos(r, &s, &c);
    if (q & 1) {
        const double t = s;
        s = c;
        c = -t;
    }
    if (q & 2) s = -s, c = -c;
    *sn = x < 0.0 ? -s : s;
    *cs = c;
}

// exp(x) (cos y + i sin y).  A zero imaginary part stays a zero of its sign (inf * sin(0) would be NaN); exp(x) beyond the
// double range is applied in two factors so that exp(x) sin(y) can stay finite (710 + 1e-3 i); an infinite or NaN
// imaginary part gives C99's results: 0 for x = -inf, (inf, NaN) for x = +inf, NaN otherwise
__device__ __forceinline__ cd2 cexp_c128(cd2 z)
{
    const double x = z.x, y = z.y;
    if (y == 0.0) return cd2{exp(x), y};
    if (!(fabs(y) <= CYB_DBL_MAX)) {
        if (x == -INFINITY) return cd2{0.0, copysign(0.0, y)};
        if (x == INFINITY) return cd2{x, __builtin_nan("")};
        return cd2{__builtin_nan(""), __builtin_nan("")};
    }
    double sn, cs;
    if (fabs(y) >= 0x1p30) sincos_large(y, &sn, &cs);
    else sincos(y, &sn, &cs);
    if (x > 709.0 && x < INFINITY) {
        const double e1 = exp(709.0), e2 = exp(x - 709.0);
        return cd2{(cs * e1) * e2, (sn * e1) * e2};
    }
    const double ex = exp(x);
    return cd2{ex * cs, ex * sn};
}

// log|z| + i arg z.  |z| near 1: log1p of |z|^2 - 1, summed without cancellation error (the squares with their FMA
// remainders), so that the real part keeps a RELATIVE accuracy (log(hypot) returns 0 for 1 + 1e-9 i, the value is 5e-19).
// Parts beyond 1e154 or below 1e-150 are scaled by 2^-+600 before the hypot.
__device__ __forceinline__ cd2 clog_c128(cd2 z)
{
    const double ax = fabs(z.x), ay = fabs(z.y);
    const double im = atan2(z.y, z.x);
    if (ax != ax || ay != ay) return cd2{(ax == INFINITY || ay == INFINITY) ? INFINITY : __builtin_nan(""), im};
    const double hi = fmax(ax, ay), lo = fmin(ax, ay);
    if (hi == INFINITY) return cd2{hi, im};
    if (hi == 0.0) return cd2{-INFINITY, im};
    const double ln2_600 = 600.0 * 0.6931471805599453;
    if (hi > 1e154) return cd2{log(hypot(hi * 0x1p-600, lo * 0x1p-600)) + ln2_600, im};
    if (hi < 1e-150) return cd2{log(hypot(hi * 0x1p600, lo * 0x1p600)) - ln2_600, im};
    if (hi >= 0.5 && hi <= 2.0) {
        // |z|^2 - 1 = 2 d + d^2 + lo^2 with d = hi - 1 (exact): the two squares as (product, FMA remainder) pairs
        const double d = hi - 1.0;
        const double p1 = mul_rn(d, d), e1 = fma(d, d, -p1);
        const double p2 = mul_rn(lo, lo), e2 = fma(lo, lo, -p2);
        const double s1 = p1 + p2, b1 = s1 - p1, r1 = (p1 - (s1 - b1)) + (p2 - b1);
        const double a = 2.0 * d, s2 = a + s1, b2 = s2 - a, r2 = (a - (s2 - b2)) + (s1 - b2);
        return cd2{0.5 * log1p(s2 + (r2 + r1 + e1 + e2)), im};
    }
    return cd2{log(hypot(hi, lo)), im};
}

// Smith's division.  A zero divisor divides each part by +0 (numpy's rule: inf / NaN per component)
__device__ __forceinline__ cd2 cdiv_c128(cd2 z, cd2 w)
{
    if (w.x == 0.0 && w.y == 0.0) return cd2{z.x / 0.0, z.y / 0.0};
    if (fabs(w.x) >= fabs(w.y)) {
        const double q = w.y / w.x, den = w.x + w.y * q;
        return cd2{(z.x + z.y * q) / den, (z.y - z.x * q) / den};
    }
    const double q = w.x / w.y, den = w.x * q + w.y;
    return cd2{(z.x * q + z.y) / den, (z.y * q - z.x) / den};
}

__global__ void __launch_bounds__(NT) celementwise_kernel(const VecDev* __restrict__ descs, const Item* __restrict__ items, int op)
{
    const Item it = items[blockIdx.x];
    const VecDev d = descs[it.desc];
    const GLOBAL_AS d2* x = (const GLOBAL_AS d2*)d.x;
    const GLOBAL_AS d2* y = (const GLOBAL_AS d2*)d.y;
    GLOBAL_AS d2* outc = (GLOBAL_AS d2*)d.out;
    gp outr = (gp)d.out;
    for (int64_t e = it.start + threadIdx.x; e < it.start + it.count; e += NT) {
        const d2 z = x[e];
        if (op == 0) {
            outr[e] = hypot(z.x, z.y);
            continue;
        }
        if (op == 4) {
            outr[e] = atan2(z.y, z.x);
            continue;
        }
        d2 r;
        switch (op) {
        case 1: r = csqrt_c128(z); break;
        case 2: r = cexp_c128(z); break;
        case 3: r = clog_c128(z); break;
        case 5: {
            // numpy's vectorised loop (fmaddsub): the products with z.y are rounded, those with z.x fused into the sum --
            // which part overflows to Inf and which to NaN depends on it, so the contraction is spelled out
            const d2 w = y[e];
            r = d2{fma(z.x, w.x, -mul_rn(z.y, w.y)), fma(z.x, w.y, mul_rn(z.y, w.x))};
            break;
        }
        default: r = cdiv_c128(z, y[e]); break;
        }
        outc[e] = r;
    }
}

// ---------------------------------------------------------------------------------------------
// elementwise
// kind 0: out = a*x + b*y (y may be null) ; kind 1: binary op ; kind 2: unary op ; kind 3: unary op with parameter a
// numpy's ``x ** y`` is exact whenever the result is representable (4.0 ** 3.0 == 64.0 is asserted by the reference's own
// test, test_block_backend_cpp.py:127); the device library's pow() is only 1-ulp accurate.  Integer exponents of moderate
// size go through exponentiation by squaring (every partial product exact in the representable cases).
__device__ __forceinline__ double pow_exactish(double x, double y)
{
    // x ** 0.5 is a correctly rounded square root in numpy; the device pow() was 5 ulp off at 1e10 ** 0.5.  pow's own edge
    // cases: (-0) ** 0.5 = +0, (-inf) ** 0.5 = +inf
    if (y == 0.5) return x == -INFINITY ? INFINITY : sqrt(x) + 0.0;
    const double yi = rint(y);
    if (yi == y && fabs(y) <= 4096.0) {
        unsigned int n = (unsigned int)fabs(yi);
        const bool n_odd = n & 1u;
        double base = x, r = 1.0;
        while (n) {
            if (n & 1u) r *= base;
            base *= base;
            n >>= 1;
        }
        // every partial product was exact or rounded once while r stayed a normal number
        if (fabs(r) >= 2.2250738585072014e-308 && fabs(r) <= 1.7976931348623157e308) return yi < 0.0 ? 1.0 / r : r;
        // r overflowed (2.0 ** -1074 is 5e-324, not 1 / inf), is denormal, zero or NaN: a power of two exactly by ldexp,
        // everything else by pow()
        int ex;
        if (frexp(fabs(x), &ex) == 0.5) {
            const double mag = ldexp(1.0, (int)((double)(ex - 1) * yi));
            return (x < 0.0 && (n_odd)) ? -mag : mag;
        }
    }
    return pow(x, y);
}

__device__ __forceinline__ void elementwise_body(const VecDev& d, const Item& it, int kind, int op, double a, double b)
{
    gcp x = (gcp)d.x;
    gcp y = (gcp)d.y;
    gp out = (gp)d.out;
    const int64_t e1 = it.start + it.count;
    if (kind == 0) { // a*x + b*y (the Krylov axpy / scale): 16-byte accesses when the three operands allow
        const bool al = ((((uintptr_t)(x + it.start)) | ((uintptr_t)(out + it.start)) | (d.y ? (uintptr_t)(y + it.start) : 0)) & 15) == 0;
        const int64_t nv = al ? it.count / 2 : 0;
        const GLOBAL_AS d2* xv2 = (const GLOBAL_AS d2*)(x + it.start);
        const GLOBAL_AS d2* yv2 = (const GLOBAL_AS d2*)(y + it.start);
        GLOBAL_AS d2* ov2 = (GLOBAL_AS d2*)(out + it.start);
        if (d.y) {
            for (int64_t i = threadIdx.x; i < nv; i += NT) {
                const d2 xa = xv2[i], ya = yv2[i];
                ov2[i] = d2{a * xa.x + b * ya.x, a * xa.y + b * ya.y};
            }
            for (int64_t e = it.start + 2 * nv + threadIdx.x; e < e1; e += NT) out[e] = a * x[e] + b * y[e];
        } else {
            for (int64_t i = threadIdx.x; i < nv; i += NT) {
                const d2 xa = xv2[i];
                ov2[i] = d2{a * xa.x, a * xa.y};
            }
            for (int64_t e = it.start + 2 * nv + threadIdx.x; e < e1; e += NT) out[e] = a * x[e];
        }
        return;
    }
    for (int64_t e = it.start + threadIdx.x; e < e1; e += NT) {
        const double xv = x[e];
        double r;
        if (kind == 0) {
            r = d.y ? a * xv + b * y[e] : a * xv;
        } else if (kind == 1) {
            const double yv = y[e];
            r = op == 0 ? xv + yv : op == 1 ? xv - yv : op == 2 ? xv * yv : op == 3 ? xv / yv : pow_exactish(xv, yv);
        } else if (kind == 3) { // unary with one parameter `a`
            switch (op) {
            case 0: r = fabs(xv) < a ? 0.0 : 1.0 / xv; break;        // cutoff_inverse
            case 1: r = xv > a ? log(xv) : 0.0; break;                // stable_log
            case 2: r = pow_exactish(xv, a); break;                   // Block::pow(Scalar)
            default: r = xv != xv ? xv : (signbit(xv) ? 3.141592653589793 : 0.0); break; // angle of a real number
            }
        } else {
            switch (op) {
            case 0: r = fabs(xv); break;
            case 1: r = sqrt(xv); break;
            case 2: r = exp(xv); break;
            case 3: r = log(xv); break;
            case 4: r = -xv; break;
            case 5: r = xv * xv; break;
            case 6: r = 1.0 / xv; break;
            case 7: r = (double)(float)xv; break;       // round to float32: the cast-on-store of float32 / complex64 blocks
            default: r = trunc(xv); break;               // int64 blocks hold integers (np.asarray(x, int64) truncates)
            }
        }
        out[e] = r;
    }
}
__global__ void __launch_bounds__(NT) elementwise_kernel(const VecDev* __restrict__ descs, const Item* __restrict__ items,
                                                         int kind, int op, double a, double b)
{
    const Item it = items[blockIdx.x];
    const VecDev d = descs[it.desc];
    elementwise_body(d, it, kind, op, a, b);
}
__global__ void __launch_bounds__(NT) elementwise_one_kernel(VecDev d, int64_t chunk, int kind, int op, double a, double b)
{   // (ONE vector: see reduce_stage1_one_kernel)
    elementwise_body(d, nth_item(chunk, d.n), kind, op, a, b);
}

struct ScaleDev {
    const double* x;
    const double* f;
    double* out;
    int64_t outer, axis, inner;
};
__global__ void __launch_bounds__(NT) scale_axis_kernel(const ScaleDev* __restrict__ descs, const Item* __restrict__ items)
{
    const Item it = items[blockIdx.x];
    const ScaleDev d = descs[it.desc];
    gcp x = (gcp)d.x;
    gcp f = (gcp)d.f;
    gp out = (gp)d.out;
    const int64_t e1 = it.start + it.count;
    // pairs of elements per thread (16-byte accesses) when both buffers are 16-byte aligned; the factor index of
    // the second element of a pair is derived from the first one's without a second division
    const bool al = ((((uintptr_t)(x + it.start)) | ((uintptr_t)(out + it.start))) & 15) == 0;
    const int64_t nv = al ? it.count / 2 : 0;
    const GLOBAL_AS d2* xv = (const GLOBAL_AS d2*)(x + it.start);
    GLOBAL_AS d2* ov = (GLOBAL_AS d2*)(out + it.start);
    for (int64_t i = threadIdx.x; i < nv; i += NT) {
        const int64_t e = it.start + 2 * i;
        const int64_t t = e / d.inner, in = e - t * d.inner;
        const int64_t j0 = t % d.axis;
        int64_t j1 = j0;
        if (in + 1 == d.inner) j1 = (j0 + 1 == d.axis) ? 0 : j0 + 1;
        const d2 v = xv[i];
        ov[i] = d2{v.x * f[j0], v.y * f[j1]};
    }
    for (int64_t e = it.start + 2 * nv + threadIdx.x; e < e1; e += NT) {
        const int64_t j = (e / d.inner) % d.axis;
        out[e] = x[e] * f[j];
    }
}

struct MaskDev {
    const double* x;
    double* out;
    const int64_t* idx;
    int64_t outer, axis, inner, n_keep;
};
// work items enumerate the elements of the SMALL side (outer, n_keep, inner)
__global__ void __launch_bounds__(NT) mask_kernel(const MaskDev* __restrict__ descs, const Item* __restrict__ items, int scatter)
{
    const Item it = items[blockIdx.x];
    const MaskDev d = descs[it.desc];
    gcp x = (gcp)d.x;
    gp out = (gp)d.out;
    const GLOBAL_AS int64_t* idx = (const GLOBAL_AS int64_t*)d.idx;
    const int64_t e1 = it.start + it.count;
    if (d.inner >= 16) {
        // row gather / scatter (the mask acts on a leading axis: Vh of a truncated SVD): every wave moves whole kept
        // rows, the kept index is decoded once per row
        const int64_t inner = d.inner;
        const int64_t r0 = it.start / inner, r1 = (e1 - 1) / inner;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int64_t row = r0 + wave; row <= r1; row += NT / 64) {
            const int64_t c0 = (row == r0) ? it.start - r0 * inner : 0;
            const int64_t c1 = (row == r1) ? e1 - r1 * inner : inner;
            const int64_t o = row / d.n_keep, j = row - o * d.n_keep;
            const int64_t big = (o * d.axis + idx[j]) * inner + c0, sm = row * inner + c0;
            const GLOBAL_AS uint64_t* sp = (const GLOBAL_AS uint64_t*)(x + (scatter ? sm : big));
            GLOBAL_AS uint64_t* dp = (GLOBAL_AS uint64_t*)(out + (scatter ? big : sm));
            wave_copy_row8(sp, dp, c1 - c0, lane);
        }
        return;
    }
    if (d.outer * d.axis * d.inner < ((int64_t)1 << 31)) {
        // short inner runs (inner = 1: the mask acts on the last axis, U of a truncated SVD): 32-bit index arithmetic
        const uint32_t inner = (uint32_t)d.inner, nk = (uint32_t)d.n_keep, axis = (uint32_t)d.axis;
        for (uint32_t e = (uint32_t)it.start + threadIdx.x; e < (uint32_t)e1; e += NT) {
            const uint32_t t = e / inner, in = e - t * inner;
            const uint32_t o = t / nk, j = t - o * nk;
            const uint32_t big = (o * axis + (uint32_t)idx[j]) * inner + in;
            if (scatter) out[big] = x[e];
            else out[e] = x[big];
        }
        return;
    }
    if ((d.inner & 1) == 0 && ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0) {
        // even inner extent: a pair of neighbours never straddles a kept slice, 16-byte accesses on both sides
        for (int64_t e = it.start + 2 * threadIdx.x; e < e1; e += 2 * NT) {
            const int64_t t = e / d.inner, in = e - t * d.inner;
            const int64_t j = t % d.n_keep, o = t / d.n_keep;
            const int64_t big = (o * d.axis + idx[j]) * d.inner + in;
            if (scatter) *(GLOBAL_AS d2*)(out + big) = *(const GLOBAL_AS d2*)(x + e);
            else *(GLOBAL_AS d2*)(out + e) = *(const GLOBAL_AS d2*)(x + big);
        }
        return;
    }
    for (int64_t e = it.start + threadIdx.x; e < e1; e += NT) {
        const int64_t in = e % d.inner;
        const int64_t t = e / d.inner;
        const int64_t j = t % d.n_keep, o = t / d.n_keep;
        const int64_t big = (o * d.axis + idx[j]) * d.inner + in;
        if (scatter) out[big] = x[e];
        else out[e] = x[big];
    }
}

__global__ void __launch_bounds__(NT) fill_kernel(double* __restrict__ out, int64_t n, double v)
{
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) out[e] = v;
}
__global__ void __launch_bounds__(NT) eye_kernel(double* __restrict__ out, int64_t n)
{
    const int64_t tot = n * n;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * NT)
        out[e] = (e / n == e % n) ? 1.0 : 0.0;
}

// Philox4x32-10 counter-based generator + Box-Muller
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0;
    c[1] = n1;
    c[2] = n2;
    c[3] = n3;
}
__global__ void __launch_bounds__(NT) random_normal_kernel(double* __restrict__ out, int64_t n, uint64_t seed, double sigma)
{
    const int64_t npair = (n + 1) / 2;
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < npair; p += (int64_t)gridDim.x * NT) {
        uint32_t c[4] = {(uint32_t)p, (uint32_t)((uint64_t)p >> 32), 0u, 0u};
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            philox_round(c, k0, k1);
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t a = ((uint64_t)c[0] << 32) | c[1];
        const uint64_t b = ((uint64_t)c[2] << 32) | c[3];
        const double u1 = ((double)(a >> 11) + 1.0) * (1.0 / 9007199254740992.0); // (0,1]
        const double u2 = (double)(b >> 11) * (1.0 / 9007199254740992.0);         // [0,1)
        const double rad = sigma * sqrt(-2.0 * log(u1));
        double s, co;
        sincos(6.283185307179586 * u2, &s, &co);
        out[2 * p] = rad * co;
        if (2 * p + 1 < n) out[2 * p + 1] = rad * s;
    }
}

__global__ void __launch_bounds__(NT) random_uniform_kernel(double* __restrict__ out, int64_t n, uint64_t seed, double lo, double hi)
{
    const int64_t npair = (n + 1) / 2;
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < npair; p += (int64_t)gridDim.x * NT) {
        uint32_t c[4] = {(uint32_t)p, (uint32_t)((uint64_t)p >> 32), 1u, 0u}; // counter word 2 separates the uniform stream
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            philox_round(c, k0, k1);
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t a = ((uint64_t)c[0] << 32) | c[1];
        const uint64_t b = ((uint64_t)c[2] << 32) | c[3];
        out[2 * p] = lo + (hi - lo) * ((double)(a >> 11) * (1.0 / 9007199254740992.0));
        if (2 * p + 1 < n) out[2 * p + 1] = lo + (hi - lo) * ((double)(b >> 11) * (1.0 / 9007199254740992.0));
    }
}

// ---------------------------------------------------------------------------------------------
// comparisons -> boolean (one byte per element) blocks, and their reductions
__global__ void __launch_bounds__(NT) compare_kernel(const double* __restrict__ x_, const double* __restrict__ y_, double scalar,
                                                     uint8_t* __restrict__ out_, int64_t n, int op)
{
    gcp x = (gcp)x_;
    gcp y = (gcp)y_;
    GLOBAL_AS uint8_t* out = (GLOBAL_AS uint8_t*)out_;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        const double a = x[e], b = y ? y[e] : scalar;
        bool r;
        switch (op) {
        case 0: r = a < b; break;
        case 1: r = a <= b; break;
        case 2: r = a > b; break;
        case 3: r = a >= b; break;
        case 4: r = a == b; break;
        default: r = a != b; break;
        }
        out[e] = r ? 1 : 0;
    }
}
__global__ void __launch_bounds__(NT) convert_u8_f64_kernel(const uint8_t* __restrict__ x_, double* __restrict__ out_, int64_t n)
{
    const GLOBAL_AS uint8_t* x = (const GLOBAL_AS uint8_t*)x_;
    gp out = (gp)out_;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) out[e] = x[e] ? 1.0 : 0.0;
}
__global__ void __launch_bounds__(NT) count_nonzero_kernel(const uint8_t* __restrict__ x_, int64_t n, unsigned long long* __restrict__ result)
{
    const GLOBAL_AS uint8_t* x = (const GLOBAL_AS uint8_t*)x_;
    unsigned long long c = 0;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) c += x[e] != 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(result, c); // integer atomics: order-independent, deterministic
}

// np.allclose as a count of violations: an element passes when x == y (equal infinities) or when both are finite and
// |x - y| <= atol + rtol * |y|; a NaN on either side fails.  cplx: interleaved (re, im) elements, |.| the complex modulus.
__global__ void __launch_bounds__(NT) allclose_count_kernel(const double* __restrict__ x_, const double* __restrict__ y_, int64_t n, int cplx,
                                                            double rtol, double atol, unsigned long long* __restrict__ result)
{
    gcp x = (gcp)x_;
    gcp y = (gcp)y_;
    const double big = 1.7976931348623157e308;
    unsigned long long c = 0;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        bool ok;
        if (cplx) {
            const d2 a = ((const GLOBAL_AS d2*)x)[e], b = ((const GLOBAL_AS d2*)y)[e];
            const bool fin = fabs(a.x) <= big && fabs(a.y) <= big && fabs(b.x) <= big && fabs(b.y) <= big;
            ok = (a.x == b.x && a.y == b.y) || (fin && hypot(a.x - b.x, a.y - b.y) <= atol + rtol * hypot(b.x, b.y));
        } else {
            const double a = x[e], b = y[e];
            ok = a == b || (fabs(a) <= big && fabs(b) <= big && fabs(a - b) <= atol + rtol * fabs(b));
        }
        c += ok ? 0 : 1;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(result, c); // integer atomics: order-independent, deterministic
}

// extremum with its flat index (ties: lowest index, like np.argmax / np.argmin): mode 0 max, 1 min, 2 max |x|.
// NaN: the key is NaN and the index that of the first NaN, in every mode (np.max / np.min / np.argmax / np.argmin)
struct Ext {
    double v;
    long long i;
};
__device__ __forceinline__ bool ext_better(double v, long long i, double bv, long long bi)
{
    if (bi < 0) return true;
    const bool vn = v != v, bn = bv != bv; // a NaN key ranks above every number (np.max / np.argmax), the first one wins
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}
__device__ __forceinline__ void ext_wave(double& v, long long& i)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const long long oi = __shfl_xor(i, o);
        if (oi >= 0 && ext_better(ov, oi, v, i)) v = ov, i = oi;
    }
}
__global__ void __launch_bounds__(NT) extremum_kernel(const double* __restrict__ x_, int64_t n, int mode, Ext* __restrict__ partial,
                                                      const Ext* __restrict__ prev, int64_t n_prev)
{
    __shared__ double sv[NT / 64];
    __shared__ long long si[NT / 64];
    gcp x = (gcp)x_;
    double bv = 0.0;
    long long bi = -1;
    if (prev) { // second stage: reduce the partial records
        for (int64_t e = threadIdx.x; e < n_prev; e += NT)
            if (prev[e].i >= 0 && ext_better(prev[e].v, prev[e].i, bv, bi)) bv = prev[e].v, bi = prev[e].i;
    } else {
        for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
            const double r = x[e];
            const double key = mode == 0 ? r : mode == 1 ? -r : fabs(r); // every mode is a maximisation of `key`
            if (ext_better(key, e, bv, bi)) bv = key, bi = e;
        }
    }
    ext_wave(bv, bi);
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = bv, si[threadIdx.x >> 6] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < NT / 64; ++q)
            if (si[q] >= 0 && ext_better(sv[q], si[q], bv, bi)) bv = sv[q], bi = si[q];
        partial[blockIdx.x] = Ext{bv, bi};
    }
}

// ---------------------------------------------------------------------------------------------
// dst[idx] = (accumulate ? dst[idx] : 0) + sum_t coeff_t * src_t[idx] over N-d strided views: the tree-block updates of
// FusionTreeBackend::apply_instructions (TreePairMapping::transform_tensor, fusion_tree_mapping.cpp:391-513):
// `tree_block = sum_I f_JI * old_block[slices_I]`, `permute_combined_matrix`, `new_block[slices] = ...` as ONE
// launch per tensor -- the permutation is in the source strides, the sub-block placement in the destination view.
struct LinDev {
    double* dst;
    int32_t ndim, accumulate, term_begin, term_end;
    int64_t total;
    int64_t shape[CYB_MAX_NDIM], ds[CYB_MAX_NDIM];
};
struct LinTerm {
    const double* src;
    double coeff;
    int64_t ss[CYB_MAX_NDIM];
};
__global__ void __launch_bounds__(NT) lincomb_strided_kernel(const LinDev* __restrict__ descs, const LinTerm* __restrict__ terms,
                                                             const Item* __restrict__ items)
{
    const Item it = items[blockIdx.x];
    const LinDev d = descs[it.desc];
    gp dst = (gp)d.dst;
    for (int64_t e = it.start + threadIdx.x; e < it.start + it.count; e += NT) {
        int64_t idx[CYB_MAX_NDIM];
        int64_t rem = e, dof = 0;
#pragma unroll
        for (int k = CYB_MAX_NDIM - 1; k >= 0; --k) {
            idx[k] = 0;
            if (k < d.ndim) {
                const int64_t q = rem / d.shape[k];
                idx[k] = rem - q * d.shape[k];
                rem = q;
                dof += idx[k] * d.ds[k];
            }
        }
        double acc = d.accumulate ? dst[dof] : 0.0;
        for (int t = d.term_begin; t < d.term_end; ++t) {
            const GLOBAL_AS LinTerm* tm = (const GLOBAL_AS LinTerm*)(terms + t);
            int64_t so = 0;
#pragma unroll
            for (int k = 0; k < CYB_MAX_NDIM; ++k)
                if (k < d.ndim) so += idx[k] * tm->ss[k];
            acc += tm->coeff * ((gcp)tm->src)[so];
        }
        dst[dof] = acc;
    }
}

// complex128 form: dst and (unless src_real) the sources are interleaved (re, im) arrays, strides in complex elements; a
// term with src_real reads a float64 array (strides in doubles) -- real data under a complex mapping (anyonic R / C
// symbols): `dtype = to_complex(dtype)` at fusion_tree_mapping.cpp:433-436
struct LinTermC {
    const double* src;
    double cr, ci;
    int32_t src_real, pad;
    int64_t ss[CYB_MAX_NDIM];
};
__global__ void __launch_bounds__(NT) lincomb_strided_c128_kernel(const LinDev* __restrict__ descs, const LinTermC* __restrict__ terms,
                                                                  const Item* __restrict__ items)
{
    const Item it = items[blockIdx.x];
    const LinDev d = descs[it.desc];
    GLOBAL_AS d2* dst = (GLOBAL_AS d2*)d.dst;
    for (int64_t e = it.start + threadIdx.x; e < it.start + it.count; e += NT) {
        int64_t idx[CYB_MAX_NDIM];
        int64_t rem = e, dof = 0;
#pragma unroll
        for (int k = CYB_MAX_NDIM - 1; k >= 0; --k) {
            idx[k] = 0;
            if (k < d.ndim) {
                const int64_t q = rem / d.shape[k];
                idx[k] = rem - q * d.shape[k];
                rem = q;
                dof += idx[k] * d.ds[k];
            }
        }
        d2 acc = d.accumulate ? dst[dof] : d2{0.0, 0.0};
        for (int t = d.term_begin; t < d.term_end; ++t) {
            const GLOBAL_AS LinTermC* tm = (const GLOBAL_AS LinTermC*)(terms + t);
            int64_t so = 0;
#pragma unroll
            for (int k = 0; k < CYB_MAX_NDIM; ++k)
                if (k < d.ndim) so += idx[k] * tm->ss[k];
            d2 x;
            if (tm->src_real) x = d2{((gcp)tm->src)[so], 0.0};
            else x = ((const GLOBAL_AS d2*)tm->src)[so];
            acc.x += tm->cr * x.x - tm->ci * x.y;
            acc.y += tm->cr * x.y + tm->ci * x.x;
        }
        dst[dof] = acc;
    }
}

// validates a vector list and cuts it: hv[i] the device form of descs[i], items over all of them
static int vec_items(const char* who, const cyb_vec_desc* descs, int64_t n, bool need_y, bool need_out, std::vector<VecDev>& hv,
                     std::vector<Item>& items)
{
    hv.resize((size_t)n);
    std::vector<int64_t> totals((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        CYB_REQUIRE(descs[i].n >= 0, "vector desc %lld: negative length", (long long)i);
        CYB_REQUIRE(descs[i].n == 0 || descs[i].x, "vector desc %lld: x is NULL", (long long)i);
        CYB_REQUIRE(!need_y || descs[i].n == 0 || descs[i].y, "vector desc %lld: y is NULL", (long long)i);
        CYB_REQUIRE(!need_out || descs[i].n == 0 || descs[i].out, "vector desc %lld: out is NULL", (long long)i);
        hv[(size_t)i] = VecDev{descs[i].x, descs[i].y, descs[i].out, descs[i].n};
        totals[(size_t)i] = descs[i].n;
    }
    CYB_CUT(who, items, totals, chunk_real(sum_of(totals)));
    return CYB_OK;
}

// shared body of the three reductions. per_entry: one result per list entry, else one total
template <class Op> static int reduce_common(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev, bool per_entry)
{
    CYB_REQUIRE(ctx && result_dev, "reduction: NULL argument");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "reduction: bad descriptor list");
    const int64_t n_groups = per_entry ? n : 1;
    if (n_groups == 0) return CYB_OK;
    if (n == 1 && descs[0].n > 0) { // ONE vector: no descriptor upload
        CYB_REQUIRE(descs[0].x, "vector desc 0: x is NULL");
        const VecDev d{descs[0].x, descs[0].y, nullptr, descs[0].n};
        const int64_t chunk = chunk_real(d.n), n_items = cdiv64(d.n, chunk);
        return two_stage<1, Op>(ctx, (size_t)n_items, nullptr, 1, result_dev, [&](double* partial) {
            hipLaunchKernelGGL(reduce_stage1_one_kernel<Op>, dim3((unsigned)n_items), dim3(NT), 0, ctx->stream, d, chunk, partial);
            return CYB_OK;
        });
    }
    std::vector<VecDev> hv;
    std::vector<Item> items;
    CYB_TRY(vec_items("reduction", descs, n, false, false, hv, items));
    // segment table for stage 2
    std::vector<int64_t> seg((size_t)n_groups + 1, 0);
    if (per_entry) {
        size_t k = 0;
        for (int64_t i = 0; i < n; ++i) {
            seg[(size_t)i] = (int64_t)k;
            while (k < items.size() && items[k].desc == i) ++k;
        }
        seg[(size_t)n] = (int64_t)items.size();
    } else {
        seg[1] = (int64_t)items.size();
    }
    // (the segment table travels with the descriptors; an all-empty list still writes its zero results)
    return with_arrays(ctx, "reduction", items.size(), arrays(hv, items, seg),
                       [&](dim3 grid, const VecDev* d_descs, const Item* d_items, const int64_t* d_seg) {
                           return two_stage<1, Op>(ctx, items.size(), d_seg, n_groups, result_dev, [&](double* partial) {
                               hipLaunchKernelGGL(reduce_stage1_kernel<Op>, grid, dim3(NT), 0, ctx->stream, d_descs, d_items, partial);
                               return CYB_OK;
                           });
                       });
}

static int elementwise_common(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, int kind, int op, double a, double b,
                              bool need_y)
{
    CYB_REQUIRE(ctx, "elementwise: ctx is NULL");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "elementwise: bad descriptor list");
    if (n == 0) return CYB_OK;
    if (n == 1 && descs[0].n > 0) { // ONE vector: no descriptor upload
        CYB_REQUIRE(descs[0].x && descs[0].out && (!need_y || descs[0].y), "vector desc 0: NULL operand");
        const VecDev d{descs[0].x, descs[0].y, descs[0].out, descs[0].n};
        const int64_t chunk = chunk_real(d.n);
        hipLaunchKernelGGL(elementwise_one_kernel, dim3((unsigned)cdiv64(d.n, chunk)), dim3(NT), 0, ctx->stream, d, chunk, kind, op, a, b);
        CYB_HIP(hipGetLastError());
        return CYB_OK;
    }
    std::vector<VecDev> hv;
    std::vector<Item> items;
    CYB_TRY(vec_items("elementwise", descs, n, need_y, true, hv, items));
    return launch(ctx, "elementwise", elementwise_kernel, arrays(hv, items), kind, op, a, b);
}

} // namespace

extern "C" {

int cyb_copy_strided_batched(cyb_ctx_t ctx, const cyb_copy_desc* descs, int64_t n, int32_t elem_size)
{
    CYB_REQUIRE(ctx, "cyb_copy_strided_batched: ctx is NULL");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "cyb_copy_strided_batched: bad descriptor list");
    CYB_REQUIRE(elem_size == 1 || elem_size == 4 || elem_size == 8 || elem_size == 16,
                "cyb_copy_strided_batched: unsupported elem_size %d", elem_size);
    if (n == 0) return CYB_OK;
    const char* who = "cyb_copy_strided_batched";
    std::vector<CopyDev> hd((size_t)n);
    std::vector<CopyT> ht;                         // descriptors that take the tiled transposing path
    std::vector<int64_t> totals((size_t)n, 0), tiles; // elements of a descriptor on the strided path, tiles of one on the tiled path
    const int64_t tsz = elem_size == 8 ? 64 : 32;  // (conj needs elem_size 16)
    for (int64_t i = 0; i < n; ++i) {
        const cyb_copy_desc& d = descs[i];
        CYB_REQUIRE(d.ndim >= 0 && d.ndim <= CYB_MAX_NDIM, "copy desc %lld: ndim %d out of range", (long long)i, d.ndim);
        CYB_REQUIRE(!d.conj || elem_size == 16, "copy desc %lld: conj needs elem_size 16", (long long)i);
        CopyDev& c = hd[(size_t)i];
        c.dst = d.dst;
        c.src = d.src;
        c.conj = d.conj;
        // drop singleton axes and merge axes that are contiguous in BOTH operands
        CYB_REQUIRE(normalize_copy(d.shape, d.dst_strides, d.src_strides, d.ndim, c), "copy desc %lld: negative extent", (long long)i);
        CYB_REQUIRE(c.total == 0 || (d.dst && d.src), "copy desc %lld: NULL pointer", (long long)i);
        static const bool no_tiled = getenv("CYB_COPY_NOTILED") != nullptr;
        CopyT t;
        int64_t ntile = 0;
        if (!no_tiled && classify_transpose(c, tsz, t, ntile)) {
            t.dst = d.dst;
            t.src = d.src;
            t.conj = d.conj;
            ht.push_back(t);
            tiles.push_back(ntile);
            continue;
        }
        totals[(size_t)i] = c.total;
    }
    std::vector<Item> items, titems;
    CYB_CUT(who, titems, tiles, tiles_per_item(tsz));
    CYB_CUT(who, items, totals, chunk_real(sum_of(totals)));
    void (*const tkernel)(const CopyT*, const Item*) = elem_size == 1   ? copy_transpose_kernel<uint8_t>
                                                       : elem_size == 4 ? copy_transpose_kernel<uint32_t>
                                                       : elem_size == 8 ? copy_transpose64_kernel
                                                                        : copy_transpose_kernel<u128>;
    void (*const kernel)(const CopyDev*, const Item*) = elem_size == 1   ? copy_strided_kernel<uint8_t>
                                                        : elem_size == 4 ? copy_strided_kernel<uint32_t>
                                                        : elem_size == 8 ? copy_strided_kernel<uint64_t>
                                                                         : copy_strided_kernel<u128>;
    CYB_TRY(launch(ctx, who, tkernel, arrays(ht, titems)));
    return launch(ctx, who, kernel, arrays(hd, items));
}

int cyb_dot_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev)
{
    return reduce_common<Sum>(ctx, descs, n, result_dev, false);
}
int cyb_dot_each_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev)
{
    return reduce_common<Sum>(ctx, descs, n, result_dev, true);
}
int cyb_maxabs_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev)
{
    return reduce_common<NanMax>(ctx, descs, n, result_dev, false);
}
int cyb_axpby_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double a, double b)
{
    return elementwise_common(ctx, descs, n, 0, 0, a, b, false);
}
int cyb_binary_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, int32_t op)
{
    CYB_REQUIRE(op >= 0 && op <= 4, "cyb_binary_batched_f64: unknown op %d", op);
    return elementwise_common(ctx, descs, n, 1, op, 0, 0, true);
}
int cyb_unary_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, int32_t op)
{
    CYB_REQUIRE(op >= 0 && op <= 8, "cyb_unary_batched_f64: unknown op %d", op);
    return elementwise_common(ctx, descs, n, 2, op, 0, 0, false);
}

int cyb_unary_param_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, int32_t op, double param)
{
    CYB_REQUIRE(op >= 0 && op <= 3, "cyb_unary_param_batched_f64: unknown op %d", op);
    return elementwise_common(ctx, descs, n, 3, op, param, 0, false);
}

int cyb_compare_f64(cyb_ctx_t ctx, const double* x, const double* y, double scalar, uint8_t* out, int64_t n, int32_t op)
{
    CYB_REQUIRE(ctx && n >= 0 && (n == 0 || (x && out)), "cyb_compare_f64: bad argument");
    CYB_REQUIRE(op >= 0 && op <= 5, "cyb_compare_f64: unknown op %d", op);
    if (n == 0) return CYB_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n, NT * 4), 4096);
    hipLaunchKernelGGL(compare_kernel, dim3(grid), dim3(NT), 0, ctx->stream, x, y, scalar, out, n, op);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_convert_u8_f64(cyb_ctx_t ctx, const uint8_t* x, double* out, int64_t n)
{
    CYB_REQUIRE(ctx && n >= 0 && (n == 0 || (x && out)), "cyb_convert_u8_f64: bad argument");
    if (n == 0) return CYB_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n, NT * 4), 4096);
    hipLaunchKernelGGL(convert_u8_f64_kernel, dim3(grid), dim3(NT), 0, ctx->stream, x, out, n);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_count_nonzero_u8(cyb_ctx_t ctx, const uint8_t* x, int64_t n, uint64_t* result_dev)
{
    CYB_REQUIRE(ctx && result_dev && n >= 0 && (n == 0 || x), "cyb_count_nonzero_u8: bad argument");
    CYB_HIP(hipMemsetAsync(result_dev, 0, sizeof(uint64_t), ctx->stream));
    if (n == 0) return CYB_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n, NT * 16), 2048);
    hipLaunchKernelGGL(count_nonzero_kernel, dim3(grid), dim3(NT), 0, ctx->stream, x, n,
                       reinterpret_cast<unsigned long long*>(result_dev));
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_allclose_count(cyb_ctx_t ctx, const double* x, const double* y, int64_t n, int32_t is_complex, double rtol, double atol,
                       uint64_t* result_dev)
{
    CYB_REQUIRE(ctx && result_dev && n >= 0 && (n == 0 || (x && y)), "cyb_allclose_count: bad argument");
    CYB_HIP(hipMemsetAsync(result_dev, 0, sizeof(uint64_t), ctx->stream));
    if (n == 0) return CYB_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n, NT * 8), 2048);
    hipLaunchKernelGGL(allclose_count_kernel, dim3(grid), dim3(NT), 0, ctx->stream, x, y, n, is_complex ? 1 : 0, rtol, atol,
                       reinterpret_cast<unsigned long long*>(result_dev));
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_extremum_f64(cyb_ctx_t ctx, const double* x, int64_t n, int32_t mode, double* result_dev)
{
    CYB_REQUIRE(ctx && result_dev && n >= 1 && x, "cyb_extremum_f64: needs a non-empty vector");
    CYB_REQUIRE(mode >= 0 && mode <= 2, "cyb_extremum_f64: unknown mode %d", mode);
    const int64_t grid = std::min<int64_t>(cdiv64(n, NT * 8), 1024);
    void* part_v = nullptr;
    CYB_TRY(ctx->workspace(sizeof(Ext) * (size_t)grid, &part_v, 2));
    Ext* part = static_cast<Ext*>(part_v);
    hipLaunchKernelGGL(extremum_kernel, dim3((unsigned)grid), dim3(NT), 0, ctx->stream, x, n, mode, part, (const Ext*)nullptr, (int64_t)0);
    // result_dev[0] = key of the extremum, result_dev[1] holds the flat index as an int64 bit pattern
    static_assert(sizeof(Ext) == 2 * sizeof(double), "Ext is written into two doubles");
    hipLaunchKernelGGL(extremum_kernel, dim3(1), dim3(NT), 0, ctx->stream, x, n, mode, reinterpret_cast<Ext*>(result_dev),
                       (const Ext*)part, grid);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_random_uniform_f64(cyb_ctx_t ctx, double* out, int64_t n, uint64_t seed, double lo, double hi)
{
    CYB_REQUIRE(ctx && (n == 0 || out) && n >= 0, "cyb_random_uniform_f64: bad argument");
    if (n == 0) return CYB_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64((n + 1) / 2, NT), 2048);
    hipLaunchKernelGGL(random_uniform_kernel, dim3(grid), dim3(NT), 0, ctx->stream, out, n, seed, lo, hi);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

extern "C++" {
template <class TermIn, class TermDev, class Fill>
static int lincomb_common(cyb_ctx_t ctx, const cyb_lincomb_desc* descs, int64_t n, const TermIn* terms, int64_t n_terms, Fill fill,
                          void (*kernel)(const LinDev*, const TermDev*, const Item*))
{
    CYB_REQUIRE(ctx, "cyb_lincomb_strided_batched: ctx is NULL");
    CYB_REQUIRE(n >= 0 && n_terms >= 0 && (n == 0 || descs) && (n_terms == 0 || terms), "cyb_lincomb_strided_batched: bad lists");
    if (n == 0) return CYB_OK;
    std::vector<LinDev> hd((size_t)n);
    std::vector<TermDev> ht((size_t)n_terms);
    std::vector<int64_t> totals((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const cyb_lincomb_desc& d = descs[i];
        CYB_REQUIRE(d.ndim >= 0 && d.ndim <= CYB_MAX_NDIM, "lincomb desc %lld: ndim %d out of range", (long long)i, d.ndim);
        CYB_REQUIRE(d.term_begin >= 0 && d.term_begin <= d.term_end && d.term_end <= n_terms,
                    "lincomb desc %lld: bad term range [%d,%d)", (long long)i, d.term_begin, d.term_end);
        LinDev& c = hd[(size_t)i];
        c.dst = d.dst;
        c.ndim = d.ndim;
        c.accumulate = d.accumulate;
        c.term_begin = d.term_begin;
        c.term_end = d.term_end;
        int64_t tot = 1;
        for (int k = 0; k < CYB_MAX_NDIM; ++k) {
            c.shape[k] = k < d.ndim ? d.shape[k] : 1;
            c.ds[k] = k < d.ndim ? d.dst_strides[k] : 0;
            CYB_REQUIRE(c.shape[k] >= 0, "lincomb desc %lld: negative extent", (long long)i);
            tot *= c.shape[k];
        }
        c.total = tot;
        CYB_REQUIRE(tot == 0 || d.dst, "lincomb desc %lld: dst is NULL", (long long)i);
        for (int32_t t = d.term_begin; t < d.term_end; ++t)
            CYB_REQUIRE(tot == 0 || terms[t].src, "lincomb term %d: src is NULL", t);
        totals[(size_t)i] = tot;
    }
    for (int64_t t = 0; t < n_terms; ++t) fill(ht[(size_t)t], terms[t]);
    std::vector<Item> items;
    CYB_CUT("cyb_lincomb_strided_batched", items, totals, chunk_real(sum_of(totals)));
    return launch(ctx, "cyb_lincomb_strided_batched", kernel, arrays(hd, ht, items));
}

} // extern "C++"

int cyb_lincomb_strided_batched_f64(cyb_ctx_t ctx, const cyb_lincomb_desc* descs, int64_t n, const cyb_lincomb_term* terms,
                                    int64_t n_terms)
{
    return lincomb_common<cyb_lincomb_term, LinTerm>(
        ctx, descs, n, terms, n_terms,
        [](LinTerm& o, const cyb_lincomb_term& t) {
            o.src = t.src;
            o.coeff = t.coeff;
            for (int k = 0; k < CYB_MAX_NDIM; ++k) o.ss[k] = t.src_strides[k];
        },
        lincomb_strided_kernel);
}

int cyb_lincomb_strided_batched_c128(cyb_ctx_t ctx, const cyb_lincomb_desc* descs, int64_t n, const cyb_lincomb_term_c128* terms,
                                     int64_t n_terms)
{
    return lincomb_common<cyb_lincomb_term_c128, LinTermC>(
        ctx, descs, n, terms, n_terms,
        [](LinTermC& o, const cyb_lincomb_term_c128& t) {
            o.src = t.src;
            o.cr = t.coeff_re;
            o.ci = t.coeff_im;
            o.src_real = t.src_real;
            o.pad = 0;
            for (int k = 0; k < CYB_MAX_NDIM; ++k) o.ss[k] = t.src_strides[k];
        },
        lincomb_strided_c128_kernel);
}

int cyb_scale_axis_batched_f64(cyb_ctx_t ctx, const cyb_scale_axis_desc* descs, int64_t n)
{
    CYB_REQUIRE(ctx, "cyb_scale_axis_batched_f64: ctx is NULL");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "cyb_scale_axis_batched_f64: bad descriptor list");
    if (n == 0) return CYB_OK;
    std::vector<ScaleDev> hd((size_t)n);
    std::vector<int64_t> totals((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const auto& d = descs[i];
        CYB_REQUIRE(d.outer >= 0 && d.axis >= 0 && d.inner >= 0, "scale_axis desc %lld: negative extent", (long long)i);
        CYB_REQUIRE(d.outer * d.axis * d.inner == 0 || (d.x && d.f && d.out), "scale_axis desc %lld: NULL pointer", (long long)i);
        hd[(size_t)i] = ScaleDev{d.x, d.f, d.out, d.outer, d.axis, d.inner};
        totals[(size_t)i] = d.outer * d.axis * d.inner;
    }
    std::vector<Item> items;
    CYB_CUT("cyb_scale_axis_batched_f64", items, totals, chunk_real(sum_of(totals)));
    return launch(ctx, "cyb_scale_axis_batched_f64", scale_axis_kernel, arrays(hd, items));
}

static int mask_common(cyb_ctx_t ctx, const cyb_mask_desc* descs, int64_t n, int scatter)
{
    CYB_REQUIRE(ctx, "mask op: ctx is NULL");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "mask op: bad descriptor list");
    if (n == 0) return CYB_OK;
    std::vector<MaskDev> hd((size_t)n);
    std::vector<int64_t> totals((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const auto& d = descs[i];
        CYB_REQUIRE(d.outer >= 0 && d.axis >= 0 && d.inner >= 0 && d.n_keep >= 0 && d.n_keep <= d.axis,
                    "mask desc %lld: bad extents", (long long)i);
        CYB_REQUIRE(d.outer * d.n_keep * d.inner == 0 || (d.x && d.out && d.idx), "mask desc %lld: NULL pointer", (long long)i);
        hd[(size_t)i] = MaskDev{d.x, d.out, d.idx, d.outer, d.axis, d.inner, d.n_keep};
        totals[(size_t)i] = d.outer * d.n_keep * d.inner;
        if (scatter && d.outer * d.axis * d.inner > 0)
            CYB_HIP(hipMemsetAsync(d.out, 0, sizeof(double) * (size_t)(d.outer * d.axis * d.inner), ctx->stream));
    }
    std::vector<Item> items;
    CYB_CUT("mask op", items, totals, chunk_real(sum_of(totals)));
    return launch(ctx, "mask op", mask_kernel, arrays(hd, items), scatter);
}

int cyb_mask_gather_batched_f64(cyb_ctx_t ctx, const cyb_mask_desc* descs, int64_t n) { return mask_common(ctx, descs, n, 0); }
int cyb_mask_scatter_batched_f64(cyb_ctx_t ctx, const cyb_mask_desc* descs, int64_t n) { return mask_common(ctx, descs, n, 1); }

int cyb_fill_f64(cyb_ctx_t ctx, double* out, int64_t n, double value)
{
    CYB_REQUIRE(ctx && (n == 0 || out) && n >= 0, "cyb_fill_f64: bad argument");
    if (n == 0) return CYB_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n, NT), 2048);
    hipLaunchKernelGGL(fill_kernel, dim3(grid), dim3(NT), 0, ctx->stream, out, n, value);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_eye_f64(cyb_ctx_t ctx, double* out, int64_t n)
{
    CYB_REQUIRE(ctx && (n == 0 || out) && n >= 0, "cyb_eye_f64: bad argument");
    if (n == 0) return CYB_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n * n, NT), 2048);
    hipLaunchKernelGGL(eye_kernel, dim3(grid), dim3(NT), 0, ctx->stream, out, n);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_random_normal_f64(cyb_ctx_t ctx, double* out, int64_t n, uint64_t seed, double sigma)
{
    CYB_REQUIRE(ctx && (n == 0 || out) && n >= 0, "cyb_random_normal_f64: bad argument");
    if (n == 0) return CYB_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64((n + 1) / 2, NT), 2048);
    hipLaunchKernelGGL(random_normal_kernel, dim3(grid), dim3(NT), 0, ctx->stream, out, n, seed, sigma);
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int cyb_complex_expand_batched_f64(cyb_ctx_t ctx, const cyb_cexpand_desc* descs, int64_t n)
{
    CYB_REQUIRE(ctx, "cyb_complex_expand_batched_f64: ctx is NULL");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "cyb_complex_expand_batched_f64: bad descriptor list");
    if (n == 0) return CYB_OK;
    std::vector<CExpandDev> hd((size_t)n);
    std::vector<int64_t> totals((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const cyb_cexpand_desc& d = descs[i];
        CYB_REQUIRE(d.K >= 0 && d.N >= 0, "complex expand desc %lld: negative extent", (long long)i);
        totals[(size_t)i] = d.K * d.N;
        CYB_REQUIRE(totals[(size_t)i] == 0 || (d.src && d.dst), "complex expand desc %lld: NULL pointer", (long long)i);
        // the kernel loads and stores whole (re, im) pairs as 16-byte accesses
        CYB_REQUIRE(totals[(size_t)i] == 0 || ((((uintptr_t)d.src) | ((uintptr_t)d.dst)) & 15) == 0,
                    "complex expand desc %lld: src and dst must be 16-byte aligned", (long long)i);
        hd[(size_t)i] = CExpandDev{d.src, d.rs, d.cs, d.K, d.N, d.dst};
    }
    std::vector<Item> items;
    CYB_CUT("cyb_complex_expand_batched_f64", items, totals, kMaxChunk);
    return launch(ctx, "cyb_complex_expand_batched_f64", complex_expand_kernel, arrays(hd, items));
}

int cyb_elementwise_batched_c128(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, int32_t op)
{
    CYB_REQUIRE(ctx, "cyb_elementwise_batched_c128: ctx is NULL");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "cyb_elementwise_batched_c128: bad descriptor list");
    CYB_REQUIRE(op >= 0 && op <= 6, "cyb_elementwise_batched_c128: unknown op %d", op);
    std::vector<VecDev> hv;
    std::vector<Item> items;
    CYB_TRY(vec_items("cyb_elementwise_batched_c128", descs, n, op >= 5, true, hv, items));
    return launch(ctx, "cyb_elementwise_batched_c128", celementwise_kernel, arrays(hv, items), op);
}

int cyb_axpby_batched_c128(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double a_re, double a_im, double b_re,
                           double b_im)
{
    CYB_REQUIRE(ctx, "cyb_axpby_batched_c128: ctx is NULL");
    CYB_REQUIRE(n >= 0 && (n == 0 || descs), "cyb_axpby_batched_c128: bad descriptor list");
    std::vector<VecDev> hv;
    std::vector<Item> items;
    CYB_TRY(vec_items("cyb_axpby_batched_c128", descs, n, false, true, hv, items));
    return launch(ctx, "cyb_axpby_batched_c128", axpby_c128_kernel, arrays(hv, items), a_re, a_im, b_re, b_im);
}

} // extern "C"
