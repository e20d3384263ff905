// Batched blocked Householder QR (see blocked_qr.h).  Replaces LAPACK dgeqrf/dorgqr behind
// scipy.linalg.qr (reference src/block_backend/numpy.cpp:1236-1245) for large blocks and is the
// preconditioner / null-space provider of the Jacobi SVD (svd_jacobi.hip).
#include "blocked_qr.h"
#include "qr_strip_chunks.h"

#include <algorithm>
#include <cstdlib>
#include <utility>

namespace cyb {
namespace {

#define GLOBAL_AS __attribute__((address_space(1)))
typedef GLOBAL_AS double* gp;
typedef const GLOBAL_AS double* gcp;
typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int PNT = 512;
constexpr int PNW = PNT / 64;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct PanelDesc {
    double* Ac;
    double* V;
    double* T;   // this panel's NBK x NBK block
    double* tau;
    int64_t ld;
    int32_t m, j0, pw, pad; // pad: PANEL_* flags
    // early stop (BqrMat::ctl): ctl[0] = 0 while the factorisation runs, else 1 + the first panel step that was skipped;
    // ctl[1] = largest squared Frobenius norm of a trailing block seen so far.  parts[0 .. n_parts): the squared norms of
    // the strips the PREVIOUS step's update wrote, i.e. of this step's trailing block A[j0:, j0:]
    double* ctl = nullptr;
    const double* parts = nullptr;
    double rel2 = 0.0;
    int32_t n_parts = 0, step = 0;
};
constexpr int PANEL_V_ZEROED = 1;       // V was zero-filled by the caller: skip the rows above the panel
constexpr int PANEL_REFLECT_ALWAYS = 2; // BqrMat::reflect_always

// Factor columns [j0, j0+pw) over rows [j0, m): reflectors into V (explicit), R entries stay in Ac,
// tau, and the panel's triangular T factor (dlarft, forward columnwise).
__global__ void __launch_bounds__(PNT) qr_panel_kernel(const PanelDesc* __restrict__ descs)
{
    __shared__ double red[PNW];
    __shared__ double s_tau, s_scale;
    __shared__ double Ts[NBK][NBK + 1];
    __shared__ double z[NBK];
    __shared__ double taus[NBK];
    const PanelDesc d = descs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    gp Ac = (gp)d.Ac;
    gp V = (gp)d.V;
    const int64_t ld = d.ld;
    const int m = d.m, j0 = d.j0, pw = d.pw;
    for (int e = tid; e < NBK * (NBK + 1); e += PNT) (&Ts[0][0])[e] = 0.0;

    for (int jj = 0; jj < pw; ++jj) {
        const int col = j0 + jj;
        gp x = Ac + (int64_t)col * ld + col; // x[0..L)
        const int L = m - col;
        double mx = 0.0;
        for (int i = 1 + tid; i < L; i += PNT) mx = fmax(mx, fabs(x[i]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        mx = 0.0;
#pragma unroll
        for (int q = 0; q < PNW; ++q) mx = fmax(mx, red[q]);
        __syncthreads();
        double ss = 0.0;
        if (mx > 1e-290) { // (a tail this small -- denormal -- is zero: 1/mx would overflow)
            const double inv = 1.0 / mx;
            for (int i = 1 + tid; i < L; i += PNT) {
                const double t = x[i] * inv;
                ss += t * t;
            }
        }
        ss = wave_sum(ss);
        if (lane == 0) red[wave] = ss;
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            for (int q = 0; q < PNW; ++q) tot += red[q];
            const double xnorm = mx * sqrt(tot);
            const double alpha = x[0];
            double t = 0.0, scale = 0.0, beta = alpha;
            if (xnorm != 0.0) {
                beta = -copysign(hypot(alpha, xnorm), alpha);
                t = (beta - alpha) / beta;
                scale = 1.0 / (alpha - beta);
            } else if ((d.pad & PANEL_REFLECT_ALWAYS) && alpha != 0.0) {
                beta = -alpha; // H = I - 2 e e^T (see BqrMat::reflect_always)
                t = 2.0;
            }
            s_tau = t;
            s_scale = scale;
            taus[jj] = t;
            ((gp)d.tau)[col] = t;
            x[0] = beta; // R[col][col]
        }
        __syncthreads();
        const double tj = s_tau, scale = s_scale;
        // explicit reflector column: zeros above, 1 on the diagonal, scaled tail below
        gp v = V + (int64_t)col * ld;
        for (int i = tid; i < m; i += PNT) {
            double val = 0.0;
            if (i == col) val = 1.0;
            else if (i > col) val = (tj != 0.0) ? x[i - col] * scale : 0.0;
            v[i] = val;
        }
        __syncthreads();
        if (tj != 0.0) {
            // apply H to the remaining panel columns, one wave per column
            for (int c = col + 1 + wave; c < j0 + pw; c += PNW) {
                gp a = Ac + (int64_t)c * ld + col;
                gcp vv = v + col;
                double dot = 0.0;
                for (int i = lane; i < L; i += 64) dot += vv[i] * a[i];
                dot = wave_sum(dot) * tj;
                for (int i = lane; i < L; i += 64) a[i] -= dot * vv[i];
            }
        }
        // z[i] = v_i . v_jj for i < jj (for the T factor)
        for (int i = wave; i < jj; i += PNW) {
            gcp vi = V + (int64_t)(j0 + i) * ld;
            double dot = 0.0;
            for (int r = col + lane; r < m; r += 64) dot += vi[r] * v[r];
            dot = wave_sum(dot);
            if (lane == 0) z[i] = dot;
        }
        __syncthreads();
        // T[0:jj, jj] = -tau_jj * T[0:jj, 0:jj] z ;  T[jj][jj] = tau_jj
        if (tid < jj) {
            double acc = 0.0;
            for (int l = tid; l < jj; ++l) acc += Ts[tid][l] * z[l];
            Ts[tid][jj] = -tj * acc;
        }
        if (tid == 0) Ts[jj][jj] = tj;
        __syncthreads();
    }
    for (int e = tid; e < NBK * NBK; e += PNT) ((gp)d.T)[e] = Ts[e / NBK][e % NBK];
}

// ---------------------------------------------------------------------------------------------
// Register-resident panel factorisation (rows of the panel <= RP_NT * RP_RPT).
// Thread t owns rows j0 + t + RP_NT*q (q < RP_RPT) of all NBK panel columns in registers.  Per
// column jj ONE fused pass gives, for every column c, the dot of the current column's tail
// x[1:] with column c's tail: c == jj -> |x[1:]|^2 (the Householder norm), c > jj -> the update
// dots, c < jj -> v_c . v_jj for the T factor.  The 32 dots are reduced with a butterfly
// reduce-scatter (17 shuffles per 16 values instead of 96) and summed over the waves in LDS:
// two barriers per column instead of ~six dependent passes over global memory.
#ifndef CYB_QR_READLANE
#define CYB_QR_READLANE 1
#endif
constexpr int RP_NT = 512;
constexpr int RP_RPT = 3;
constexpr int RP_NW = RP_NT / 64;

__device__ __forceinline__ double dshfl_xor(double v, int m) { return __shfl_xor(v, m); }

#ifndef CYB_QR_REDUCE_DPP
#define CYB_QR_REDUCE_DPP 1
#endif
#if CYB_QR_REDUCE_DPP
// The same reduce-scatter without the LDS crossbar and without selects (the panel kernels are bound by their instruction
// count: ~150 instructions per call in the ds_bpermute form below, ~70 here):
//   * 64 -> 32 and 32 -> 16 lanes: v_permlane32_swap / v_permlane16_swap (gfx950) exchange the upper half (the odd rows) of one
//     register with the lower half (the even rows) of another -- after the swap a plain add IS keep + partner's send;
//   * 16 -> 8 and 8 -> 4 lanes: two DPP moves with complementary bank masks (row_mirror / row_half_mirror: involutions that pair
//     the lower with the upper half) build keep-or-partner in one register and partner-or-keep in the other; their sum is the result;
//   * inside a quad: quad_perm all-reduce.
// Same result lanes and value indices as the form below; the order of the additions differs.
__device__ __forceinline__ void dswap32(double& a, double& b)
{
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    a = __hiloint2double((int)hi[0], (int)lo[0]);
    b = __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void dswap16(double& a, double& b)
{
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    a = __hiloint2double((int)hi[0], (int)lo[0]);
    b = __hiloint2double((int)hi[1], (int)lo[1]);
}
template <int CTRL, int BANKS>
__device__ __forceinline__ double ddpp(double old, double src)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xf, BANKS, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xf, BANKS, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double reduce_scatter16(double (&v)[16], int /*lane*/)
{
    double a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double x = v[i], y = v[i + 8];
        dswap32(x, y); // lanes < 32: (own v[i], partner's v[i]);  lanes >= 32: (partner's v[i+8], own v[i+8])
        a[i] = x + y;
    }
    double b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double x = a[i], y = a[i + 4];
        dswap16(x, y); // even rows: value i of both rows of the pair;  odd rows: value i + 4
        b[i] = x + y;
    }
    constexpr int ROW_MIRROR = 0x140, ROW_HALF_MIRROR = 0x141;
    double c[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        // lanes 0-7 of a row (banks 0, 1) collect b[i], lanes 8-15 (banks 2, 3) collect b[i + 2]
        const double p = ddpp<ROW_MIRROR, 0xc>(b[i], b[i + 2]);     // 0-7: own b[i]          8-15: partner's b[i + 2]
        const double q = ddpp<ROW_MIRROR, 0x3>(b[i + 2], b[i]);     // 0-7: partner's b[i]    8-15: own b[i + 2]
        c[i] = p + q;
    }
    // lanes with (lane & 4) == 0 (banks 0, 2) collect c[0], the others (banks 1, 3) c[1]
    const double p = ddpp<ROW_HALF_MIRROR, 0xa>(c[0], c[1]);
    const double q = ddpp<ROW_HALF_MIRROR, 0x5>(c[1], c[0]);
    double d = p + q;
    d += ddpp<0x4e, 0xf>(d, d); // quad_perm [2, 3, 0, 1]
    d += ddpp<0xb1, 0xf>(d, d); // quad_perm [1, 0, 3, 2]
    return d;
}
#else
// reduce 16 per-lane values over the 64 lanes; on return lanes with (lane & 3) == 0 hold the total of
// value index ((lane>>5)&1)*8 + ((lane>>4)&1)*4 + ((lane>>3)&1)*2 + ((lane>>2)&1)
__device__ __forceinline__ double reduce_scatter16(double (&v)[16], int lane)
{
    double a[8];
    {
        const bool hi = (lane & 32) != 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double send = hi ? v[i] : v[i + 8];
            const double keep = hi ? v[i + 8] : v[i];
            a[i] = keep + dshfl_xor(send, 32);
        }
    }
    double b[4];
    {
        const bool hi = (lane & 16) != 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double send = hi ? a[i] : a[i + 4];
            const double keep = hi ? a[i + 4] : a[i];
            b[i] = keep + dshfl_xor(send, 16);
        }
    }
    double c[2];
    {
        const bool hi = (lane & 8) != 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double send = hi ? b[i] : b[i + 2];
            const double keep = hi ? b[i + 2] : b[i];
            c[i] = keep + dshfl_xor(send, 8);
        }
    }
    double d;
    {
        const bool hi = (lane & 4) != 0;
        const double send = hi ? c[0] : c[1];
        const double keep = hi ? c[1] : c[0];
        d = keep + dshfl_xor(send, 4);
    }
    d += dshfl_xor(d, 2);
    d += dshfl_xor(d, 1);
    return d;
}
#endif

struct PanelShared {
    double wred[2][RP_NW][NBK]; // per-wave partial dots, double buffered by the parity of the step
    // broadcast rows of a column step, double buffered by the parity of the step: a thread that is
    // still in step j reads buffer j & 1 while the fast ones already fill (j + 1) & 1, so a step
    // needs only two barriers
    double wsum[2][NBK];     // dots of column j's tail with every column's tail
    double rowb[2][NBK];     // the pivot row of the panel (all columns)
    double Zs[NBK][NBK + 1]; // Zs[c][j] = v_c . v_j (c < j): input of the T recurrence, built at the end
    double taus[NBK];
    double Ts[NBK][NBK + 1];
};

// One column step with a compile-time column index (every register index is static).
template <int JJ, int RPT, int NT>
__device__ __forceinline__ void panel_step(double (&P)[RPT][NBK], PanelShared& sh, const PanelDesc& d, int tid)
{
    if (JJ >= d.pw) return; // uniform
    const int lane = tid & 63, wave = tid >> 6;
    const int j0 = d.j0;
    const int prow = j0 + JJ; // pivot row
    constexpr int pb = JJ & 1;
    // ---- fused pass: dots of column JJ's tail (rows > prow) with every column's tail
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double part[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) part[c] = 0.0;
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            // (row j0 + tid + NT * q lies at or above the pivot row j0 + JJ only for q == 0 and tid <= JJ: said so explicitly,
            //  the kernel is bound by its instruction count -- ~900 per column step and wave -- and the compiler cannot see it)
            const double x = (q == 0 && tid <= JJ) ? 0.0 : P[q][JJ];
#pragma unroll
            for (int c = 0; c < 16; ++c) part[c] += x * P[q][h * 16 + c];
        }
        const double r = reduce_scatter16(part, lane);
        if ((lane & 3) == 0) {
            const int idx = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
            sh.wred[pb][wave][h * 16 + idx] = r;
        }
    }
    // the owner of the pivot row publishes it (always thread JJ, its first row)
    if (tid == JJ) {
#pragma unroll
        for (int c = 0; c < NBK; ++c) sh.rowb[pb][c] = P[0][c];
    }
    __syncthreads();
#if CYB_QR_READLANE
    // ONE barrier per column: lane c (mod 32) of EVERY wave sums the per-wave partials of column c itself and reads
    // the pivot row's entry c (nine LDS reads in flight together); the scalars of the reflector then come from lane JJ
    // by v_readlane instead of a second round through LDS
    const int lc = lane & (NBK - 1);
    double ws = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) ws += sh.wred[pb][w][lc];
    const double rb = sh.rowb[pb][lc];
    const double alpha = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(rb), JJ), __builtin_amdgcn_readlane(__double2loint(rb), JJ));
    const double xn2_raw = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(ws), JJ), __builtin_amdgcn_readlane(__double2loint(ws), JJ));
#else
    if (tid < NBK) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) t += sh.wred[pb][w][tid];
        sh.wsum[pb][tid] = t;
    }
    __syncthreads();
    // ---- reflector (every thread computes the scalars redundantly from LDS)
    const double alpha = sh.rowb[pb][JJ];
    const double xn2_raw = sh.wsum[pb][JJ];
#endif
    // PANEL_REFLECT_ALWAYS: a floor of 1e-40 alpha^2 on the squared tail norm turns the exactly-zero tail into the ordinary
    // case with beta = -alpha, tau = 2, v_tail = 0, and changes nothing else (branch-free: an extra branch here costs the
    // register kernel 28 B of scratch; relative to alpha, so that a zero column keeps tau = 0)
    const double xn2 = fma(alpha * alpha, (d.pad & PANEL_REFLECT_ALWAYS) ? 1e-40 : 0.0, xn2_raw);
    double tau = 0.0, scale = 0.0, beta = alpha;
    // (a squared tail norm in the denormal range is zero for the purpose: 1 / (alpha - beta) would overflow and
    //  the reflector would lose its orthogonality -- an exactly rank-deficient block, e.g. all ones, gets there
    //  because every elimination step leaves a trailing block 1e-16 times smaller than the one before)
    if (xn2 > 1e-290) {
        beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
        tau = (beta - alpha) / beta;
        scale = 1.0 / (alpha - beta);
    }
    // ---- update my rows: v = x*scale below the pivot, 1 on it, 0 above; columns c > JJ get H applied.
    //      Column-outer order: the broadcast factor of a column is read from LDS once, not per row.
    double v[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const double x = P[q][JJ];
        if (q == 0) { // (only a thread's first row can be the pivot row or lie above it)
            const bool below = tid > JJ;
            const bool pivot = tid == JJ;
            v[q] = below ? x * scale : (pivot ? 1.0 : 0.0);
            P[q][JJ] = below ? v[q] : (pivot ? beta : x);
        } else {
            v[q] = x * scale;
            P[q][JJ] = v[q];
        }
    }
#if CYB_QR_READLANE
    // every lane c < 32 forms the factor of column c once (ONE round trip to LDS for all columns); the update loop
    // then takes it from lane c with v_readlane -- a scalar operand, no LDS latency per column
    const double tl = tau * (rb + scale * ws);
    const int tlo = __double2loint(tl), thi = __double2hiint(tl);
#pragma unroll
    for (int c = JJ + 1; c < NBK; ++c) {
        const double t = __hiloint2double(__builtin_amdgcn_readlane(thi, c), __builtin_amdgcn_readlane(tlo, c));
#pragma unroll
        for (int q = 0; q < RPT; ++q) P[q][c] -= t * v[q]; // (columns beyond pw hold zeros and zero factors)
    }
#else
#pragma unroll
    for (int c = JJ + 1; c < NBK; ++c) {
        // v . a_c = a_c[pivot] + scale * (x_tail . a_c_tail); columns beyond pw hold zeros
        // (the uniform guard also keeps the scheduler from hoisting every column's broadcast loads at
        //  once: without it the kernel spills -- the panel already fills the register file)
        if (c < d.pw) {
            const double t = tau * (sh.rowb[pb][c] + scale * sh.wsum[pb][c]);
#pragma unroll
            for (int q = 0; q < RPT; ++q) P[q][c] -= t * v[q];
        }
    }
#endif
    // ---- inputs of the T factor: z_c = v_c . v_JJ = v_c[pivot] + scale * (v_c_tail . x_tail), c < JJ
#if CYB_QR_READLANE
    if (tid < JJ) sh.Zs[tid][JJ] = rb + scale * ws; // (tid < 32: lane tid holds column tid)
#else
    if (tid < JJ) sh.Zs[tid][JJ] = sh.rowb[pb][tid] + scale * sh.wsum[pb][tid];
#endif
    if (tid == 0) {
        sh.taus[JJ] = tau;
        ((gp)d.tau)[prow] = tau;
    }
    // no barrier here: the broadcast rows are double buffered
}

template <int RPT, int NT, int... Is>
__device__ __forceinline__ void panel_steps(double (&P)[RPT][NBK], PanelShared& sh, const PanelDesc& d, int tid,
                                            std::integer_sequence<int, Is...>)
{
    (panel_step<Is, RPT, NT>(P, sh, d, tid), ...);
}

// RPT rows per thread, NT threads: 3 x 512 for panels of up to 1536 rows, 3 x 64 / 128 / 256 for the short ones
template <int RPT, int NT = RP_NT>
__device__ __forceinline__ void panel_reg_body(const PanelDesc& d, PanelShared& sh, const int tid)
{
    gp Ac = (gp)d.Ac;
    gp V = (gp)d.V;
    const int64_t ld = d.ld;
    const int m = d.m, j0 = d.j0, pw = d.pw;
    // ---- load my rows of the panel.  Branch-free: rows beyond m / columns beyond pw load a valid element (row j0 / column
    //      pw - 1) and are zeroed by a select -- the guarded form cost 18 instructions per element, and these kernels are bound
    //      by their instruction count
    double P[RPT][NBK];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int row = j0 + tid + NT * q;
        const bool ok = row < m;
        gcp src = (gcp)Ac + (int64_t)j0 * ld + (ok ? row : j0);
#pragma unroll
        for (int c = 0; c < NBK; ++c) P[q][c] = src[(int64_t)(c < pw ? c : pw - 1) * ld];
#pragma unroll
        for (int c = 0; c < NBK; ++c) {
            asm volatile("" : "+v"(P[q][c])); // (keeps the loads unconditional and in flight together: the compiler would sink each under its select again)
            P[q][c] = (ok && c < pw) ? P[q][c] : 0.0;
        }
    }
    for (int e = tid; e < NBK * (NBK + 1); e += NT) (&sh.Zs[0][0])[e] = 0.0;
    __syncthreads();

    panel_steps<RPT, NT>(P, sh, d, tid, std::make_integer_sequence<int, NBK>{});
    // ---- write back: Ac (R above / on the diagonal, v below) and the explicit V (1 on the diagonal, 0 above: only a
    //      thread's first row, j0 + tid with tid < NBK, can be on or above the diagonal of the panel)
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int row = j0 + tid + NT * q;
        if (row < m) {
            gp pa = Ac + (int64_t)j0 * ld + row;
            gp pv = V + (int64_t)j0 * ld + row;
#pragma unroll
            for (int c = 0; c < NBK; ++c)
                if (c < pw) {
                    pa[(int64_t)c * ld] = P[q][c];
                    pv[(int64_t)c * ld] = (q > 0 || tid > c) ? P[q][c] : (tid == c ? 1.0 : 0.0);
                }
        }
    }
    // rows above the panel's first row are zero in V
    for (int64_t e = tid; e < ((d.pad & PANEL_V_ZEROED) ? 0 : (int64_t)j0 * pw); e += NT) { // (d.pad: V was zero-filled by the caller)
        const int c = (int)(e / j0), row = (int)(e % j0);
        V[(int64_t)(j0 + c) * ld + row] = 0.0;
    }
    __syncthreads();
    // ---- T factor (compact WY, T upper triangular): column j = -tau_j T[:, :j] z_j.  Row i of T only
    //      needs row i of the earlier columns, so lane i builds its own row with no exchange.
    if (tid < NBK) {
        double trow[NBK];
#pragma unroll
        for (int j = 0; j < NBK; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < j; ++l) acc += trow[l] * sh.Zs[l][j]; // (trow[l] is zero for l < tid: T is upper triangular)
            const double tj = j < pw ? sh.taus[j] : 0.0;
            trow[j] = (tid < j) ? -tj * acc : (tid == j ? tj : 0.0);
            sh.Ts[tid][j] = trow[j];
        }
    }
    __syncthreads();

    for (int e = tid; e < NBK * NBK; e += NT) ((gp)d.T)[e] = sh.Ts[e / NBK][e % NBK];
}

// Early stop of a factorisation whose trailing block has fallen to the rounding level of the matrix (a rank-deficient block:
// every block of a two-site theta = A.B): the remaining panels would factor noise.  The panel kernel of step p sums the
// squared norms of the strips step p - 1 wrote (fixed order: deterministic) -- that is ||A[j0:, j0:]||_F^2 -- and, once it
// is below rel2 x the largest such norm seen, marks the matrix stopped: this and all later panel and strip launches of the
// matrix return at once, T stays zero (the caller's zeroed workspace), so those reflectors are the identity.
// Returns true if the workgroup is to leave.  `red`: NT / 64 doubles of LDS.
template <int NT, typename Desc>
__device__ __forceinline__ bool panel_stop_check(const Desc& d, double* red, int tid, bool writer = true)
{
    if (!d.ctl) return false;
    gp ctl = (gp)d.ctl;
    const double stopped = ctl[0];
    if (stopped != 0.0) return (double)d.step >= stopped - 1.0;
    if (d.n_parts <= 0) return false;
    gcp parts = (gcp)d.parts;
    double t = 0.0;
    for (int i = tid; i < d.n_parts; i += NT) t += parts[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if ((tid & 63) == 0) red[tid >> 6] = t;
    __syncthreads();
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) sum += red[w];
    const double ref = fmax(ctl[1], sum);
    const bool stop = sum <= d.rel2 * ref;
    __syncthreads(); // (everybody has read ctl before it changes)
    if (tid == 0 && writer) {
        if (stop) ctl[0] = (double)d.step + 1.0;
        else ctl[1] = ref;
    }
    return stop;
}

__global__ void __launch_bounds__(RP_NT) qr_panel_reg_kernel(const PanelDesc* __restrict__ descs)
{
    __shared__ PanelShared sh;
    const PanelDesc d = descs[blockIdx.x];
    if (panel_stop_check<RP_NT>(d, &sh.wsum[0][0], (int)threadIdx.x)) return;
    panel_reg_body<RP_RPT>(d, sh, (int)threadIdx.x);
}
// ---------------------------------------------------------------------------------------------
// Panels of more than RP_NT * RP_RPT = 1536 rows: the register-resident factorisation spread over several workgroups
// (workgroup w owns rows j0 + 1536 w ...), which exchange their partial column dots once per column step through device
// memory -- write-through stores, one ticket per column, a bounded poll by one lane -- instead of the global-memory
// panel kernel (six dependent passes over the panel per column: 1.7 ms per panel at 2884 rows).  The pivot rows of a panel
// (j0 .. j0 + 31) always belong to workgroup 0, which sends the pivot row along with its dots.
struct PanelDescM {
    double* Ac;
    double* V;
    double* T;
    double* tau;
    double* xchg;         // [NBK column steps][n_wg][64]: 32 partial dots (+ the pivot row from workgroup 0)
    unsigned int* ticket; // [NBK], zeroed before the launch
    unsigned int* err;    // set if a poll ran out of time (partner workgroup not resident)
    int64_t ld;
    int32_t m, j0, pw, vzero;
    int32_t wg, n_wg, pad0, pad1;
    // early stop, as in PanelDesc (every workgroup of the matrix sums the same numbers in the same order and takes the same
    // decision; workgroup 0 records it)
    double* ctl = nullptr;
    const double* parts = nullptr;
    double rel2 = 0.0;
    int32_t n_parts = 0, step = 0;
};
constexpr int RPM_ROWS = RP_NT * RP_RPT;

template <int JJ>
__device__ __forceinline__ void panel_step_multi(double (&P)[RP_RPT][NBK], PanelShared& sh, const PanelDescM& d, int tid)
{
    if (JJ >= d.pw) return; // uniform
    const int lane = tid & 63, wave = tid >> 6;
    const int j0 = d.j0, rbase = d.j0 + d.wg * RPM_ROWS;
    const int prow = j0 + JJ;
    constexpr int pb = JJ & 1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double part[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) part[c] = 0.0;
#pragma unroll
        for (int q = 0; q < RP_RPT; ++q) {
            const int row = rbase + tid + RP_NT * q;
            const double x = (row <= prow) ? 0.0 : P[q][JJ];
#pragma unroll
            for (int c = 0; c < 16; ++c) part[c] += x * P[q][h * 16 + c];
        }
        const double r = reduce_scatter16(part, lane);
        if ((lane & 3) == 0) {
            const int idx = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
            sh.wred[pb][wave][h * 16 + idx] = r;
        }
    }
#pragma unroll
    for (int q = 0; q < RP_RPT; ++q)
        if (rbase + tid + RP_NT * q == prow) {
#pragma unroll
            for (int c = 0; c < NBK; ++c) sh.rowb[pb][c] = P[q][c];
        }
    __syncthreads();
    if (tid < NBK) { // (one wave: the stores of these lanes, one drain, one ticket, one poll, the loads)
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < RP_NW; ++w) t += sh.wred[pb][w][tid];
        double* slot = d.xchg + ((size_t)JJ * d.n_wg + d.wg) * 64;
        __hip_atomic_store(slot + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (d.wg == 0) __hip_atomic_store(slot + 32 + tid, sh.rowb[pb][tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) {
            // (relaxed on purpose: the data went out as write-through stores that this wave has drained, and comes in through
            //  agent-scope loads that bypass the L2 -- a release / acquire pair here would write back and invalidate the whole
            //  L2 of the XCD on every column step: 1.7 ms per panel instead of 0.3)
            __hip_atomic_fetch_add(d.ticket + JJ, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long t0 = wall_clock64();
            while (__hip_atomic_load(d.ticket + JJ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned int)d.n_wg) {
                if (wall_clock64() - t0 > 100000000ull || __hip_atomic_load(d.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { // 1 s at 100 MHz
                    __hip_atomic_store(d.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
        }
        // compiler-only barrier: the relaxed loads below must not be hoisted above the poll of lane 0 (nothing in the C++
        // memory model orders relaxed accesses to different addresses; costs no instruction and no L2 write-back)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        double tot = 0.0;
        for (int w = 0; w < d.n_wg; ++w)
            tot += __hip_atomic_load(d.xchg + ((size_t)JJ * d.n_wg + w) * 64 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh.wsum[pb][tid] = tot;
        sh.rowb[pb][tid] = __hip_atomic_load(d.xchg + (size_t)JJ * d.n_wg * 64 + 32 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const double alpha = sh.rowb[pb][JJ];
    const double xn2 = fma(alpha * alpha, (d.vzero & PANEL_REFLECT_ALWAYS) ? 1e-40 : 0.0, sh.wsum[pb][JJ]);
    double tau = 0.0, scale = 0.0, beta = alpha;
    if (xn2 > 1e-290) {
        beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
        tau = (beta - alpha) / beta;
        scale = 1.0 / (alpha - beta);
    }
    double v[RP_RPT];
#pragma unroll
    for (int q = 0; q < RP_RPT; ++q) {
        const int row = rbase + tid + RP_NT * q;
        const double x = P[q][JJ];
        const bool below = row > prow;
        const bool pivot = row == prow;
        v[q] = below ? x * scale : (pivot ? 1.0 : 0.0);
        P[q][JJ] = below ? v[q] : (pivot ? beta : x);
    }
#pragma unroll
    for (int c = JJ + 1; c < NBK; ++c) {
        if (c < d.pw) {
            const double t = tau * (sh.rowb[pb][c] + scale * sh.wsum[pb][c]);
#pragma unroll
            for (int q = 0; q < RP_RPT; ++q) P[q][c] -= t * v[q];
        }
    }
    if (tid < JJ) sh.Zs[tid][JJ] = sh.rowb[pb][tid] + scale * sh.wsum[pb][tid];
    if (tid == 0) {
        sh.taus[JJ] = tau;
        if (d.wg == 0) ((gp)d.tau)[prow] = tau;
    }
}

template <int... Is>
__device__ __forceinline__ void panel_steps_multi(double (&P)[RP_RPT][NBK], PanelShared& sh, const PanelDescM& d, int tid,
                                                  std::integer_sequence<int, Is...>)
{
    (panel_step_multi<Is>(P, sh, d, tid), ...);
}

__global__ void __launch_bounds__(RP_NT) qr_panel_multi_kernel(const PanelDescM* __restrict__ descs)
{
    __shared__ PanelShared sh;
    const PanelDescM d = descs[blockIdx.x];
    const int tid = threadIdx.x;
    if (panel_stop_check<RP_NT>(d, &sh.wsum[0][0], tid, d.wg == 0)) return;
    gp Ac = (gp)d.Ac;
    gp V = (gp)d.V;
    const int64_t ld = d.ld;
    const int m = d.m, j0 = d.j0, pw = d.pw, rbase = d.j0 + d.wg * RPM_ROWS;
    double P[RP_RPT][NBK];
#pragma unroll
    for (int q = 0; q < RP_RPT; ++q) {
        const int row = rbase + tid + RP_NT * q;
#pragma unroll
        for (int c = 0; c < NBK; ++c) P[q][c] = (row < m && c < pw) ? Ac[(int64_t)(j0 + c) * ld + row] : 0.0;
    }
    for (int e = tid; e < NBK * (NBK + 1); e += RP_NT) (&sh.Zs[0][0])[e] = 0.0;
    __syncthreads();
    panel_steps_multi(P, sh, d, tid, std::make_integer_sequence<int, NBK>{});
#pragma unroll
    for (int q = 0; q < RP_RPT; ++q) {
        const int row = rbase + tid + RP_NT * q;
        if (row < m) {
#pragma unroll
            for (int c = 0; c < NBK; ++c)
                if (c < pw) {
                    const int col = j0 + c;
                    Ac[(int64_t)col * ld + row] = P[q][c];
                    V[(int64_t)col * ld + row] = (row > col) ? P[q][c] : (row == col ? 1.0 : 0.0);
                }
        }
    }
    if (d.wg == 0 && !(d.vzero & PANEL_V_ZEROED))
        for (int64_t e = tid; e < (int64_t)j0 * pw; e += RP_NT) {
            const int c = (int)(e / j0), row = (int)(e % j0);
            V[(int64_t)(j0 + c) * ld + row] = 0.0;
        }
    __syncthreads();
    if (tid < NBK) {
        double trow[NBK];
#pragma unroll
        for (int j = 0; j < NBK; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < j; ++l) acc += trow[l] * sh.Zs[l][j]; // (trow[l] is zero for l < tid: T is upper triangular)
            const double tj = j < pw ? sh.taus[j] : 0.0;
            trow[j] = (tid < j) ? -tj * acc : (tid == j ? tj : 0.0);
            sh.Ts[tid][j] = trow[j];
        }
    }
    __syncthreads();
    if (d.wg == 0)
        for (int e = tid; e < NBK * NBK; e += RP_NT) ((gp)d.T)[e] = sh.Ts[e / NBK][e % NBK];
}

// Panels of at most RP_WAVE_ROWS rows (every panel of a DMRG-sized block, the last panels of a large one): the same
// body on ONE wave -- the per-column reduction over eight waves through LDS and the workgroup barrier behind it, which
// is most of a column step at these sizes, shrink to a wave-local exchange.
constexpr int RP_WAVE_RPT = 3;
constexpr int RP_WAVE_ROWS = 64 * RP_WAVE_RPT;
__global__ void __launch_bounds__(64) qr_panel_wave_kernel(const PanelDesc* __restrict__ descs)
{
    __shared__ PanelShared sh;
    const PanelDesc d = descs[blockIdx.x];
    if (panel_stop_check<64>(d, &sh.wsum[0][0], (int)threadIdx.x)) return;
    panel_reg_body<RP_WAVE_RPT, 64>(d, sh, (int)threadIdx.x);
}
// ... and on two / four waves for up to 2 / 4 * RP_WAVE_ROWS rows (the sectors of a chi = 512 bond; the later panels of a
// large block): the fewer waves take part in the per-column reduction and barrier, the shorter the column step.
// (Tall panels on four waves with six rows per thread were measured too: the 192 panel doubles per thread spill --
//  228 B of scratch -- and the chi=4096 step goes from 36.7 to 40.3 ms; four rows per thread for panels up to 1024 rows:
//  neutral, 36.5 / 36.6 vs 36.6 / 36.3 ms.  Panels above 768 rows keep eight waves x 3 rows.)
__global__ void __launch_bounds__(128) qr_panel_wave2_kernel(const PanelDesc* __restrict__ descs)
{
    __shared__ PanelShared sh;
    const PanelDesc d = descs[blockIdx.x];
    if (panel_stop_check<128>(d, &sh.wsum[0][0], (int)threadIdx.x)) return;
    panel_reg_body<RP_WAVE_RPT, 128>(d, sh, (int)threadIdx.x);
}
__global__ void __launch_bounds__(256) qr_panel_wave4_kernel(const PanelDesc* __restrict__ descs)
{
    __shared__ PanelShared sh;
    const PanelDesc d = descs[blockIdx.x];
    if (panel_stop_check<256>(d, &sh.wsum[0][0], (int)threadIdx.x)) return;
    panel_reg_body<RP_WAVE_RPT, 256>(d, sh, (int)threadIdx.x);
}

// ---------------------------------------------------------------------------------------------
// Block-reflector application to one 32-column strip, ONE launch per panel step for the whole batch:
//     C_s <- (I - V P V^T) C_s,   P = T (apply Q) or T^T (apply Q^T, the trailing update of the factorisation).
// A strip is private to its workgroup, so the three products of the compact-WY update chain inside the
// kernel instead of across launches (the grouped-GEMM formulation this replaced needed two launches per panel
// step, ~34 us each at the chi=4096 sizes, almost all of it launch + tail latency of narrow problems):
//   1. W1 = V^T C_s   (32 x 32, K = rows): f64 MFMA 16x16x4, K split over the eight waves, both operands are
//      read as row PAIRS of a column (the two k-steps of a pair use the same pairing on both sides);
//   2. W2 = P W1      (32 x 32 x 32) from LDS, one 16 x 16 tile per wave;
//   3. C_s^T -= W2^T V^T, 16 rows of C_s per MFMA tile in the TRANSPOSED form, so that the lanes of a
//      load/store run along the rows of the column-major strip (coalesced), W2 stays in registers.
// Algorithmic traffic: C_s read twice (the second time from L2/MALL) and written once, V read twice.
struct StripDesc {
    double* C;       // strip: element (i, c) at C[c*ldc + i], i < mr, c < nc
    const double* V; // reflector panel: (i, a) at V[a*ldv + i], i < mr, a < pw
    const double* T; // NBK x NBK row-major, zero outside the leading pw x pw block
    int64_t ldc, ldv;
    int32_t mr, nc, pw, transT;
    // early stop (see panel_stop_check): a strip of panel step `step` returns at once if the matrix was stopped at or before
    // that step; a factorisation strip leaves the squared norm of the rows it wrote BELOW the panel's pw rows in *part_out
    const double* ctl = nullptr;
    double* part_out = nullptr;
    int32_t step = 0, pad2 = 0;
};
constexpr int ST_NT = 512; // two waves per SIMD: the loads of one hide behind the MFMAs of the other
constexpr int ST_NW = ST_NT / 64;
constexpr int ST_LS = NBK + 1;
constexpr int ST_UN = 4;

// NORM: the strips also leave the squared norm of what they wrote (early stop; a separate instantiation -- the accumulator
// costs the kernel 20 B of scratch, which the plain strips must not pay)
template <bool NORM>
__global__ void __launch_bounds__(ST_NT) reflector_strip_kernel(const StripDesc* __restrict__ descs)
{
    __shared__ double part[ST_NW][NBK][ST_LS];
    __shared__ double W1s[NBK][ST_LS], W2s[NBK][ST_LS], Ps[NBK][ST_LS];
    const StripDesc d = descs[blockIdx.x];
    if (d.ctl) { // (workgroup-uniform)
        const double stopped = *(gcp)d.ctl;
        if (stopped != 0.0 && (double)d.step >= stopped - 1.0) return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, kq = lane >> 4;
    gcp V = (gcp)d.V;
    gp C = (gp)d.C;
    gcp T = (gcp)d.T;
    const int mr = d.mr, nc = d.nc, pw = d.pw;
    const int64_t ldv = d.ldv, ldc = d.ldc;
    for (int e = tid; e < NBK * NBK; e += ST_NT) {
        const int a = e / NBK, b = e % NBK;
        Ps[a][b] = T[d.transT ? b * NBK + a : e];
    }
    // ---- phase 1: partial W1 of this wave's row chunks (8 rows per step).  Columns beyond pw / nc are
    //      clamped to column 0: their products meet zero rows/columns of P or are never stored.
    {
        const int64_t vo0 = (int64_t)(x < pw ? x : 0) * ldv, vo1 = (int64_t)(x + 16 < pw ? x + 16 : 0) * ldv;
        const int64_t co0 = (int64_t)(x < nc ? x : 0) * ldc, co1 = (int64_t)(x + 16 < nc ? x + 16 : 0) * ldc;
        d4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
        const int nstep = (mr + 7) / 8;
        double va[ST_UN][2][2], ca[ST_UN][2][2], vn[ST_UN][2][2], cn[ST_UN][2][2]; // [step][tile][row of the pair]
        auto load = [&](double (&v)[ST_UN][2][2], double (&c)[ST_UN][2][2], int s0) {
#pragma unroll
            for (int u = 0; u < ST_UN; ++u) {
                const int i = (s0 + ST_NW * u) * 8 + 2 * kq;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bool ok = i + h < mr;
                    const int ii = ok ? i + h : 0;
                    v[u][0][h] = ok ? V[vo0 + ii] : 0.0;
                    v[u][1][h] = ok ? V[vo1 + ii] : 0.0;
                    c[u][0][h] = ok ? C[co0 + ii] : 0.0;
                    c[u][1][h] = ok ? C[co1 + ii] : 0.0;
                }
            }
        };
        if (wave < nstep) load(va, ca, wave);
        for (int s0 = wave; s0 < nstep; s0 += ST_NW * ST_UN) {
            const bool more = s0 + ST_NW * ST_UN < nstep;
            if (more) load(vn, cn, s0 + ST_NW * ST_UN);
#pragma unroll
            for (int u = 0; u < ST_UN; ++u) {
                if (s0 + ST_NW * u < nstep) { // wave-uniform (rows beyond mr inside a step are loaded as zeros)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int j = 0; j < 2; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u][i][h], ca[u][j][h], acc[i][j], 0, 0, 0);
                }
            }
            if (more) {
#pragma unroll
                for (int u = 0; u < ST_UN; ++u)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            va[u][i][h] = vn[u][i][h];
                            ca[u][i][h] = cn[u][i][h];
                        }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) part[wave][i * 16 + kq + 4 * r][j * 16 + x] = acc[i][j][r];
    }
    __syncthreads();
    for (int e = tid; e < NBK * NBK; e += ST_NT) {
        const int a = e / NBK, c = e % NBK;
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < ST_NW; ++w) t += part[w][a][c];
        W1s[a][c] = t;
    }
    __syncthreads();
    // ---- phase 2: W2 = P W1, tile (wave >> 1, wave & 1)
    if (wave < 4) {
        const int ta = wave >> 1, tc = wave & 1;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < NBK / 4; ++kk)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ps[ta * 16 + x][4 * kk + kq], W1s[4 * kk + kq][tc * 16 + x], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) W2s[ta * 16 + kq + 4 * r][tc * 16 + x] = acc[r];
    }
    __syncthreads();
    // ---- phase 3: (C_s)^T tile [c][i] -= sum_a W2[a][c] V[i][a], 16 rows i per tile, tiles dealt to the waves
    {
        double w2[2][NBK / 4];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int kk = 0; kk < NBK / 4; ++kk) w2[ct][kk] = -W2s[4 * kk + kq][ct * 16 + x];
        int64_t vcol[NBK / 4], ccol[2][4];
#pragma unroll
        for (int kk = 0; kk < NBK / 4; ++kk) vcol[kk] = (int64_t)(4 * kk + kq < pw ? 4 * kk + kq : 0) * ldv;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = ct * 16 + kq + 4 * r;
                ccol[ct][r] = (int64_t)(c < nc ? c : 0) * ldc;
            }
        const int ntile = (mr + 15) / 16;
        struct Tile {
            double v[NBK / 4];
            d4 c[2];
        };
        auto load = [&](Tile& t, int rt) {
            const int i = rt * 16 + x;
            const bool ok = i < mr;
            const int ii = ok ? i : 0;
#pragma unroll
            for (int kk = 0; kk < NBK / 4; ++kk) t.v[kk] = ok ? V[vcol[kk] + ii] : 0.0;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) t.c[ct][r] = C[ccol[ct][r] + ii];
        };
        double nrm2 = 0.0; // squared norm of the entries this lane writes below the panel's rows
        auto finish = [&](Tile& t, int rt) {
#pragma unroll
            for (int kk = 0; kk < NBK / 4; ++kk) {
                t.c[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w2[0][kk], t.v[kk], t.c[0], 0, 0, 0);
                t.c[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w2[1][kk], t.v[kk], t.c[1], 0, 0, 0);
            }
            const int i = rt * 16 + x;
            if (i < mr) {
                const double below = i >= pw ? 1.0 : 0.0;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (ct * 16 + kq + 4 * r < nc) {
                            C[ccol[ct][r] + i] = t.c[ct][r];
                            if constexpr (NORM) nrm2 = fma(below * t.c[ct][r], t.c[ct][r], nrm2);
                        }
            }
        };
        // three tiles in rotation: two are in flight while one is multiplied (a tile is ~0.4 us of MFMA, a miss ~1-2 us)
        Tile t0, t1, t2;
        if (wave < ntile) load(t0, wave);
        if (wave + ST_NW < ntile) load(t1, wave + ST_NW);
        for (int rt = wave; rt < ntile; rt += 3 * ST_NW) {
            if (rt + 2 * ST_NW < ntile) load(t2, rt + 2 * ST_NW);
            finish(t0, rt);
            if (rt + ST_NW < ntile) {
                if (rt + 3 * ST_NW < ntile) load(t0, rt + 3 * ST_NW);
                finish(t1, rt + ST_NW);
            }
            if (rt + 2 * ST_NW < ntile) {
                if (rt + 4 * ST_NW < ntile) load(t1, rt + 4 * ST_NW);
                finish(t2, rt + 2 * ST_NW);
            }
        }
        if constexpr (NORM) if (d.part_out) { // (workgroup-uniform) fixed reduction order: lanes, then waves
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nrm2 += __shfl_xor(nrm2, o);
            __syncthreads(); // (W1s is free: phase 2 is over)
            if (lane == 0) W1s[0][wave] = nrm2;
            __syncthreads();
            if (tid == 0) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < ST_NW; ++w) t += W1s[0][w];
                *(gp)d.part_out = t;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The same update with the ROWS of a strip split over several workgroups, in two launches (round 3).  A strip workgroup of
// reflector_strip_kernel is a latency chain -- its eight waves stream 1442 rows in ~6 dependent batches of loads per phase,
// ~38 us whatever the rest of the chip does, and a panel step of a large matrix has only ~45 strips for 256 CUs.  Here a
// strip of mr rows becomes ceil(mr / chunk) workgroups of at most `chunk` rows (default 384):
//   strip_w1_kernel    : partial W1 = V_chunk^T C_chunk (phase 1 of the strip kernel on the chunk's rows) -> wpart[slot];
//   strip_apply_kernel : W1 = sum of the strip's partials (fixed order), W2 = P W1, C_chunk^T -= W2^T V_chunk^T (phases 2, 3).
// One batch of loads per phase instead of six; the launch boundary between the two replaces an exchange inside a launch.
struct ChunkDesc {
    double* C;       // the chunk's rows of the strip: element (i, c) at C[c*ldc + i], i < mr, c < nc
    const double* V; // the same rows of the reflector panel
    const double* T;
    double* wpart;   // partial W1's of the strip: n_slots x NBK*NBK doubles
    int64_t ldc, ldv;
    int32_t mr, nc, pw, transT;
    int32_t slot, n_slots, row0, step; // row0: first row of the chunk inside the strip (the rows below pw count for the stop test)
    const double* ctl;
    double* part_out;
};

__global__ void __launch_bounds__(ST_NT) strip_w1_kernel(const ChunkDesc* __restrict__ descs)
{
    __shared__ double part[ST_NW][NBK][ST_LS];
    const ChunkDesc d = descs[blockIdx.x];
    if (d.ctl) { // (workgroup-uniform)
        const double stopped = *(gcp)d.ctl;
        if (stopped != 0.0 && (double)d.step >= stopped - 1.0) return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, kq = lane >> 4;
    gcp V = (gcp)d.V;
    gp C = (gp)d.C;
    const int mr = d.mr, nc = d.nc, pw = d.pw;
    const int64_t ldv = d.ldv, ldc = d.ldc;
    // ---- phase 1: partial W1 of this wave's row chunks (8 rows per step).  Columns beyond pw / nc are
    //      clamped to column 0: their products meet zero rows/columns of P or are never stored.
    {
        const int64_t vo0 = (int64_t)(x < pw ? x : 0) * ldv, vo1 = (int64_t)(x + 16 < pw ? x + 16 : 0) * ldv;
        const int64_t co0 = (int64_t)(x < nc ? x : 0) * ldc, co1 = (int64_t)(x + 16 < nc ? x + 16 : 0) * ldc;
        d4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
        const int nstep = (mr + 7) / 8;
        double va[ST_UN][2][2], ca[ST_UN][2][2], vn[ST_UN][2][2], cn[ST_UN][2][2]; // [step][tile][row of the pair]
        auto load = [&](double (&v)[ST_UN][2][2], double (&c)[ST_UN][2][2], int s0) {
#pragma unroll
            for (int u = 0; u < ST_UN; ++u) {
                const int i = (s0 + ST_NW * u) * 8 + 2 * kq;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bool ok = i + h < mr;
                    const int ii = ok ? i + h : 0;
                    v[u][0][h] = ok ? V[vo0 + ii] : 0.0;
                    v[u][1][h] = ok ? V[vo1 + ii] : 0.0;
                    c[u][0][h] = ok ? C[co0 + ii] : 0.0;
                    c[u][1][h] = ok ? C[co1 + ii] : 0.0;
                }
            }
        };
        if (wave < nstep) load(va, ca, wave);
        for (int s0 = wave; s0 < nstep; s0 += ST_NW * ST_UN) {
            const bool more = s0 + ST_NW * ST_UN < nstep;
            if (more) load(vn, cn, s0 + ST_NW * ST_UN);
#pragma unroll
            for (int u = 0; u < ST_UN; ++u) {
                if (s0 + ST_NW * u < nstep) { // wave-uniform (rows beyond mr inside a step are loaded as zeros)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int j = 0; j < 2; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u][i][h], ca[u][j][h], acc[i][j], 0, 0, 0);
                }
            }
            if (more) {
#pragma unroll
                for (int u = 0; u < ST_UN; ++u)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            va[u][i][h] = vn[u][i][h];
                            ca[u][i][h] = cn[u][i][h];
                        }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) part[wave][i * 16 + kq + 4 * r][j * 16 + x] = acc[i][j][r];
    }
    __syncthreads();
    gp out = (gp)d.wpart + (size_t)d.slot * (NBK * NBK);
    for (int e = tid; e < NBK * NBK; e += ST_NT) {
        const int a = e / NBK, c = e % NBK;
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < ST_NW; ++w) t += part[w][a][c];
        out[e] = t;
    }
}

template <bool NORM>
__global__ void __launch_bounds__(ST_NT) strip_apply_kernel(const ChunkDesc* __restrict__ descs)
{
    __shared__ double W1s[NBK][ST_LS], W2s[NBK][ST_LS], Ps[NBK][ST_LS];
    const ChunkDesc d = descs[blockIdx.x];
    if (d.ctl) { // (workgroup-uniform)
        const double stopped = *(gcp)d.ctl;
        if (stopped != 0.0 && (double)d.step >= stopped - 1.0) return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, kq = lane >> 4;
    gcp V = (gcp)d.V;
    gp C = (gp)d.C;
    gcp T = (gcp)d.T;
    const int mr = d.mr, nc = d.nc, pw = d.pw;
    const int64_t ldv = d.ldv, ldc = d.ldc;
    gcp wp = (gcp)d.wpart;
    for (int e = tid; e < NBK * NBK; e += ST_NT) {
        const int a = e / NBK, b = e % NBK;
        Ps[a][b] = T[d.transT ? b * NBK + a : e];
        double t = 0.0;
        for (int sl = 0; sl < d.n_slots; ++sl) t += wp[(size_t)sl * (NBK * NBK) + e]; // (the same order in every chunk of the strip)
        W1s[a][b] = t;
    }
    __syncthreads();
    // ---- phase 2: W2 = P W1, tile (wave >> 1, wave & 1)
    if (wave < 4) {
        const int ta = wave >> 1, tc = wave & 1;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < NBK / 4; ++kk)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ps[ta * 16 + x][4 * kk + kq], W1s[4 * kk + kq][tc * 16 + x], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) W2s[ta * 16 + kq + 4 * r][tc * 16 + x] = acc[r];
    }
    __syncthreads();
    // ---- phase 3: (C_s)^T tile [c][i] -= sum_a W2[a][c] V[i][a], 16 rows i per tile, tiles dealt to the waves
    {
        double w2[2][NBK / 4];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int kk = 0; kk < NBK / 4; ++kk) w2[ct][kk] = -W2s[4 * kk + kq][ct * 16 + x];
        int64_t vcol[NBK / 4], ccol[2][4];
#pragma unroll
        for (int kk = 0; kk < NBK / 4; ++kk) vcol[kk] = (int64_t)(4 * kk + kq < pw ? 4 * kk + kq : 0) * ldv;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = ct * 16 + kq + 4 * r;
                ccol[ct][r] = (int64_t)(c < nc ? c : 0) * ldc;
            }
        const int ntile = (mr + 15) / 16;
        struct Tile {
            double v[NBK / 4];
            d4 c[2];
        };
        auto load = [&](Tile& t, int rt) {
            const int i = rt * 16 + x;
            const bool ok = i < mr;
            const int ii = ok ? i : 0;
#pragma unroll
            for (int kk = 0; kk < NBK / 4; ++kk) t.v[kk] = ok ? V[vcol[kk] + ii] : 0.0;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) t.c[ct][r] = C[ccol[ct][r] + ii];
        };
        double nrm2 = 0.0; // squared norm of the entries this lane writes below the panel's rows
        auto finish = [&](Tile& t, int rt) {
#pragma unroll
            for (int kk = 0; kk < NBK / 4; ++kk) {
                t.c[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w2[0][kk], t.v[kk], t.c[0], 0, 0, 0);
                t.c[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w2[1][kk], t.v[kk], t.c[1], 0, 0, 0);
            }
            const int i = rt * 16 + x;
            if (i < mr) {
                const double below = i + d.row0 >= pw ? 1.0 : 0.0; // (row index inside the strip)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (ct * 16 + kq + 4 * r < nc) {
                            C[ccol[ct][r] + i] = t.c[ct][r];
                            if constexpr (NORM) nrm2 = fma(below * t.c[ct][r], t.c[ct][r], nrm2);
                        }
            }
        };
        // three tiles in rotation: two are in flight while one is multiplied (a tile is ~0.4 us of MFMA, a miss ~1-2 us)
        Tile t0, t1, t2;
        if (wave < ntile) load(t0, wave);
        if (wave + ST_NW < ntile) load(t1, wave + ST_NW);
        for (int rt = wave; rt < ntile; rt += 3 * ST_NW) {
            if (rt + 2 * ST_NW < ntile) load(t2, rt + 2 * ST_NW);
            finish(t0, rt);
            if (rt + ST_NW < ntile) {
                if (rt + 3 * ST_NW < ntile) load(t0, rt + 3 * ST_NW);
                finish(t1, rt + ST_NW);
            }
            if (rt + 2 * ST_NW < ntile) {
                if (rt + 4 * ST_NW < ntile) load(t1, rt + 4 * ST_NW);
                finish(t2, rt + 2 * ST_NW);
            }
        }
        if constexpr (NORM) if (d.part_out) { // (workgroup-uniform) fixed reduction order: lanes, then waves
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nrm2 += __shfl_xor(nrm2, o);
            __syncthreads(); // (W1s is free: phase 2 is over)
            if (lane == 0) W1s[0][wave] = nrm2;
            __syncthreads();
            if (tid == 0) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < ST_NW; ++w) t += W1s[0][w];
                *(gp)d.part_out = t;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Merged T factor of a GROUP of consecutive panels (the wide application of Q, see bqr_apply_q): the w <= W reflector
// columns of the group act as ONE block reflector I - V_S T_S V_S^T with T_S (w x w, upper triangular) built from the
// stored 32 x 32 factors T_b on its diagonal and, for the block column b at offset a,
//     T_S[0:a, a:a+w_b] = -T_S[0:a, 0:a] (V_S[:, 0:a]^T V_S[:, a:a+w_b]) T_b .
// The Gram blocks come from a grouped-GEMM launch (n_gp row-chunk partials, summed here in a fixed order); one workgroup
// per group runs the dependent block columns.  Every entry of the W x W image is written (the workspace is not zeroed).
struct MergeDesc {
    const double* G;  // n_gp partial Gram images, W x W row-major each (only the blocks above the block diagonal are set)
    const double* T;  // the group's first stored panel factor; panel b at T + b * NBK * NBK
    double* TS;       // W x W row-major
    int64_t g_stride; // doubles between two partials
    int32_t w, W, n_gp, pad;
};
constexpr int MG_NT = 256;
// AMAX: rows of the largest left factor T_S[0:a, 0:a], W - 32.  Up to 96 (W <= 128) the finished part of T_S stays in LDS; a
// 256-wide group reads it back from its global image (its workgroup wrote it: same CU, write-through L1).
template <int AMAX>
__global__ void __launch_bounds__(MG_NT) merge_t_kernel(const MergeDesc* __restrict__ descs)
{
    constexpr bool TS_LDS = AMAX <= 96;
    __shared__ double Gs[AMAX][NBK + 1], X[AMAX][NBK + 1];
    __shared__ double Tb[NBK][NBK + 1];
    __shared__ double TSs[TS_LDS ? AMAX : 1][TS_LDS ? AMAX + 1 : 1];
    const MergeDesc d = descs[blockIdx.x];
    const int tid = threadIdx.x;
    const int W = d.W, w = d.w;
    gcp G = (gcp)d.G;
    gcp T = (gcp)d.T;
    gp TS = (gp)d.TS;
    for (int e = tid; e < W * W; e += MG_NT) {
        const int r = e / W, c = e % W;
        double v = 0.0;
        if (r / NBK == c / NBK && r < w && c < w) v = T[(size_t)(r / NBK) * (NBK * NBK) + (r % NBK) * NBK + (c % NBK)];
        TS[e] = v;
        if constexpr (TS_LDS)
            if (r < AMAX && c < AMAX) TSs[r][c] = v;
    }
    const int nb = (w + NBK - 1) / NBK;
    for (int b = 1; b < nb; ++b) {
        const int a = b * NBK, wb = min(NBK, w - a);
        __syncthreads(); // (the part of T_S written so far is visible to the whole workgroup; Gs, X and Tb are free)
        for (int e = tid; e < NBK * NBK; e += MG_NT) Tb[e / NBK][e % NBK] = T[(size_t)b * (NBK * NBK) + e];
        for (int e = tid; e < a * NBK; e += MG_NT) { // the Gram block, partials summed in a fixed order
            const int i = e / NBK, l = e % NBK;
            double g = 0.0;
            if (l < wb)
                for (int p = 0; p < d.n_gp; ++p) g += G[(size_t)p * d.g_stride + (size_t)i * W + a + l];
            Gs[i][l] = g;
        }
        __syncthreads();
        // X = G[0:a, a:a+wb] T_b
        for (int e = tid; e < a * NBK; e += MG_NT) {
            const int i = e / NBK, c = e % NBK;
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < NBK; ++l) acc += Gs[i][l] * Tb[l][c];
            X[i][c] = acc;
        }
        __syncthreads();
        // T_S[0:a, a:a+wb] = -T_S[0:a, 0:a] X   (T_S[0:a, 0:a] is upper triangular)
        for (int e = tid; e < a * NBK; e += MG_NT) {
            const int i = e / NBK, c = e % NBK;
            double acc = 0.0;
            if constexpr (TS_LDS) {
                for (int l = i; l < a; ++l) acc += TSs[i][l] * X[l][c];
            } else {
                for (int l = i; l < a; ++l) acc += TS[(size_t)i * W + l] * X[l][c];
            }
            if (c < wb) {
                TS[(size_t)i * W + a + c] = -acc;
                if constexpr (TS_LDS)
                    if (a + c < AMAX) TSs[i][a + c] = -acc;
            }
        }
    }
}

// W1 = sum of its row-chunk partials, in place of the first (the wide application sums them once here instead of carrying
// every partial as a K-segment of the update: the update is the larger of the two products)
struct SumDesc {
    double* W1;     // partial s at W1 + s * stride
    int64_t n, stride;
    int32_t ns, pad;
};
__global__ void __launch_bounds__(256) sum_partials_kernel(const SumDesc* __restrict__ descs)
{
    const SumDesc d = descs[blockIdx.y];
    gp W1 = (gp)d.W1;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < d.n; e += (int64_t)gridDim.x * 256) {
        double t = W1[e];
        for (int sidx = 1; sidx < d.ns; ++sidx) t += W1[e + (int64_t)sidx * d.stride];
        W1[e] = t;
    }
}

inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }

__global__ void __launch_bounds__(256) xpose_kernel(const XposeDesc* __restrict__ descs)
{
    __shared__ double tile[32][33];
    __shared__ int cidx[32]; // source columns of a tile (XposeDesc::idx): one load per column, not one per element
    const XposeDesc d = descs[blockIdx.y];
    gcp in = (gcp)d.in;
    gp out = (gp)d.out;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (d.plain) {
        const int64_t tot = (int64_t)d.R * d.C;
        for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
            const int64_t r = e / d.C, c = e % d.C;
            out[r * d.ldo + c] = in[(d.idx ? (int64_t)d.idx[r] : r) * d.ldi + c];
        }
        return;
    }
    const int tr = (d.R + 31) / 32, tc = (d.C + 31) / 32;
    for (int t = blockIdx.x; t < tr * tc; t += gridDim.x) {
        const int r0 = (t / tc) * 32, c0 = (t % tc) * 32;
        __syncthreads();
        if (d.idx) { // (uniform over the workgroup)
            if (threadIdx.x < 32) cidx[threadIdx.x] = c0 + (int)threadIdx.x < d.C ? d.idx[c0 + threadIdx.x] : 0;
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) { // read in[c*ldi + r]: r contiguous
            const int c = c0 + ty + 8 * q, r = r0 + tx;
            tile[ty + 8 * q][tx] = (c < d.C && r < d.R) ? in[(int64_t)(d.idx ? cidx[ty + 8 * q] : c) * d.ldi + r] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) { // write out[r*ldo + c]: c contiguous
            const int r = r0 + ty + 8 * q, c = c0 + tx;
            if (r < d.R && c < d.C) {
                double v = tile[tx][ty + 8 * q];
                if (d.upper && (r > c || r >= d.rlim)) v = 0.0;
                out[(int64_t)r * d.ldo + c] = v;
            }
        }
    }
}

__global__ void __launch_bounds__(256) eye_cols_kernel(const EyeDesc* __restrict__ descs)
{
    const EyeDesc d = descs[blockIdx.y];
    gp C = (gp)d.C;
    const int64_t tot = (int64_t)d.m * d.kc;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
        const int64_t c = e / d.m, i = e % d.m;
        C[c * d.ld + i] = (i == c + d.col0) ? 1.0 : 0.0;
    }
}

} // namespace

int xpose_batched(cyb_ctx_t ctx, const std::vector<XposeDesc>& descs)
{
    if (descs.empty()) return CYB_OK;
    void* d = nullptr;
    CYB_TRY(ctx->upload(descs.data(), sizeof(XposeDesc) * descs.size(), &d));
    hipLaunchKernelGGL(xpose_kernel, dim3(helper_grid_x(descs.size()), (unsigned)descs.size()), dim3(256), 0, ctx->stream, static_cast<const XposeDesc*>(d));
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

int eye_cols_batched(cyb_ctx_t ctx, const std::vector<EyeDesc>& descs)
{
    if (descs.empty()) return CYB_OK;
    void* d = nullptr;
    CYB_TRY(ctx->upload(descs.data(), sizeof(EyeDesc) * descs.size(), &d));
    hipLaunchKernelGGL(eye_cols_kernel, dim3(64, (unsigned)descs.size()), dim3(256), 0, ctx->stream, static_cast<const EyeDesc*>(d));
    CYB_HIP(hipGetLastError());
    return CYB_OK;
}

// The long-K product of a block-reflector application, W1 = V^T A (NBK x nt, K = remaining rows), has
// only nt/32 narrow tiles, each a serial walk over K: it is cut into up to kWSplit row chunks that
// run as independent problems, and the partials are summed for free as K-segments of the small
// product with T that follows (W2 = T^T sum_s W1_s = sum_s T^T W1_s).
constexpr int kWSplit = 8;
static inline int w_split(int64_t mr)
{
    static const int env = getenv("CYB_QR_WSPLIT") ? atoi(getenv("CYB_QR_WSPLIT")) : 0;
    if (env > 0) return (int)std::min<int64_t>(std::min(env, kWSplit), std::max<int64_t>(1, (mr + 255) / 256));
    // measured on the chi=4096 SVD list (1442 rows): 1 chunk 56.6 ms, 2: 53.1, 4: 53.6, 8: 55.1 -- every chunk
    // is one more K-segment of the rank-32 update that follows
    return mr >= 2600 ? 4 : mr >= 1800 ? 3 : mr >= 700 ? 2 : 1;
}

static void add_strips(std::vector<StripDesc>& out, double* C, int64_t ldc, int64_t ncols, const double* V, int64_t ldv,
                       const double* T, int64_t mr, int pw, int transT)
{
    for (int64_t c0 = 0; c0 < ncols; c0 += NBK)
        out.push_back(StripDesc{C + (size_t)c0 * ldc, V, T, ldc, ldv, (int32_t)mr, (int32_t)std::min<int64_t>(NBK, ncols - c0), pw, transT});
}

// ---- row-split strips (strip_w1_kernel + strip_apply_kernel): the chunk arithmetic is in qr_strip_chunks.h
static int strip_split_mode()
{
    // CYB_QR_CHUNK_ROWS: unset / -1 = adaptive, 0 = never split, n = fixed chunk rows (multiple of 16)
    static const int v = getenv("CYB_QR_CHUNK_ROWS") ? atoi(getenv("CYB_QR_CHUNK_ROWS")) : -1;
    return v < 0 ? -1 : v / 16 * 16;
}
int bqr_strip_slots(int64_t rows) { return strip_slot_bound(rows, strip_split_mode()); }
// chunk rows of a panel step whose strips are (rows, count) pairs; 0: whole strips (the one-launch strip kernel)
static int step_chunk_rows(const std::vector<std::pair<int, int>>& strips, int n_cu)
{
    static const int ch_min = getenv("CYB_QR_CHUNK_MIN") ? atoi(getenv("CYB_QR_CHUNK_MIN")) : kChunkRowsMin;
    return choose_chunk_rows(strips, n_cu, strip_split_mode(), ch_min);
}
// the partial-W1 workspace of the row-split strips (slot 4): n_slots x NBK * NBK doubles, or null when the strips are never split
static int split_workspace(cyb_ctx_t ctx, size_t n_slots, double** out)
{
    *out = nullptr;
    if (strip_split_mode() == 0) return CYB_OK;
    void* w = nullptr;
    CYB_TRY(ctx->workspace(sizeof(double) * NBK * NBK * std::max<size_t>(n_slots, 1), &w, 4));
    *out = static_cast<double*>(w);
    return CYB_OK;
}

// one more 256-byte aligned piece of a host image that goes up in one upload; returns its offset
static size_t put(std::vector<char>& image, const void* src, size_t bytes)
{
    const size_t off = al256(image.size());
    image.resize(off + bytes);
    memcpy(image.data() + off, src, bytes);
    return off;
}

// Panel steps are staged, uploaded and launched in CHUNKS of 2, 6, 18, ... steps: the host builds the next chunk while the
// device runs the previous ones.  With one image for the whole factorisation the device sat idle for the 0.30-0.36 ms it
// takes to lay out 46 steps of a 15-matrix list (kernel trace of the chi=4096 step: the gap in front of the first panel
// kernel of either QR).  for (StepChunks c(n); c.more(); c.next()) covers steps [c.begin, c.end) of n.
struct StepChunks {
    int n, begin = 0, len = 2, end;
    explicit StepChunks(int n_steps) : n(n_steps), end(std::min(n_steps, 2)) {}
    bool more() const { return begin < n; }
    void next()
    {
        begin += len;
        len *= 3;
        end = std::min(n, begin + len);
    }
};

// The block-reflector update of ONE panel step for the whole batch, staged into the step's host image and launched from
// its device copy: the row-split pair strip_w1_kernel + strip_apply_kernel when the step's strips are cut into chunks,
// else the one-launch reflector_strip_kernel.
struct StripStep {
    size_t off_sd = 0, off_cd = 0;
    unsigned n_sd = 0, n_cd = 0;
    bool norm = false; // some strip leaves its squared norm for the early-stop test (the instantiations with the accumulator)
    // ch: the step's chunk rows (step_chunk_rows, 0: whole strips; the caller's, because bqr_factor lays out part_out by them), wsplit: the partial-W1 workspace
    void stage(std::vector<StripDesc>& sd, int ch, double* wsplit, std::vector<char>& image)
    {
        if (sd.empty()) return;
        // longest strips first: the launch is one wave of workgroups, the tail is the longest strip
        std::stable_sort(sd.begin(), sd.end(), [](const StripDesc& a, const StripDesc& b) { return a.mr > b.mr; });
        n_sd = (unsigned)sd.size();
        off_sd = put(image, sd.data(), sizeof(StripDesc) * sd.size());
        if (ch <= 0) return;
        std::vector<ChunkDesc> cd;
        size_t slot_base = 0;
        for (const StripDesc& d : sd) {
            const int nch = strip_chunks(d.mr, ch);
            for (int sl = 0; sl < nch; ++sl) {
                const StripChunk c = strip_chunk(d.mr, ch, sl);
                cd.push_back(ChunkDesc{d.C + c.row0, d.V + c.row0, d.T, wsplit + slot_base * (size_t)(NBK * NBK), d.ldc, d.ldv, c.rows, d.nc, d.pw,
                                       d.transT, sl, nch, c.row0, d.step, d.ctl, d.part_out ? d.part_out + sl : nullptr});
            }
            slot_base += (size_t)nch;
        }
        n_cd = (unsigned)cd.size();
        off_cd = put(image, cd.data(), sizeof(ChunkDesc) * cd.size());
    }
    int launch(cyb_ctx_t ctx, const void* d_image) const
    {
        if (!n_sd) return CYB_OK;
        const char* base = static_cast<const char*>(d_image);
        const ChunkDesc* cdp = reinterpret_cast<const ChunkDesc*>(base + off_cd);
        const StripDesc* sdp = reinterpret_cast<const StripDesc*>(base + off_sd);
        if (n_cd) {
            hipLaunchKernelGGL(strip_w1_kernel, dim3(n_cd), dim3(ST_NT), 0, ctx->stream, cdp);
            if (norm) hipLaunchKernelGGL(strip_apply_kernel<true>, dim3(n_cd), dim3(ST_NT), 0, ctx->stream, cdp);
            else hipLaunchKernelGGL(strip_apply_kernel<false>, dim3(n_cd), dim3(ST_NT), 0, ctx->stream, cdp);
        } else if (norm)
            hipLaunchKernelGGL(reflector_strip_kernel<true>, dim3(n_sd), dim3(ST_NT), 0, ctx->stream, sdp);
        else
            hipLaunchKernelGGL(reflector_strip_kernel<false>, dim3(n_sd), dim3(ST_NT), 0, ctx->stream, sdp);
        CYB_HIP(hipGetLastError());
        return CYB_OK;
    }
};

// ---- wide application of Q (bqr_apply_q): switches, read once per process
//   CYB_QR_APPLY_WIDE   unset: the shape rule below; 0: strips for every target; 1: wide for every target with more than one panel
//   CYB_QR_APPLY_WIDTH  reflector columns per group: 64, 128 (default) or 256
static int wide_mode()
{
    static const int v = getenv("CYB_QR_APPLY_WIDE") ? (atoi(getenv("CYB_QR_APPLY_WIDE")) != 0 ? 1 : 0) : -1;
    return v;
}
static int wide_width()
{
    static const int v = [] {
        const int e = getenv("CYB_QR_APPLY_WIDTH") ? atoi(getenv("CYB_QR_APPLY_WIDTH")) : 128;
        return (e == 64 || e == 256) ? e : 128;
    }();
    return v;
}
constexpr int64_t kWideMinK = 256, kWideMinKc = 256, kWideMinCols = 4096;
// The shape rule: reflector columns of the matrix, columns of the target -- never data.  A target with fewer than kWideMinK
// reflector columns has at most one full group: the three launches that build the merged factors cost more than the panel
// steps they replace.  And the W1 product of a group has only W x (columns of all wide targets of the call) outputs: below
// kWideMinCols columns (bqr_apply_q) it cannot fill the chip and the row-split strips win -- measured: one 1442^2 theta block
// 18.2 ms on strips, 19.0 wide; the chi = 1024 list (three targets, 1030 columns) 4.75 ms against 5.2; the 15-block chi = 4096
// list (8462 columns) 25.1 against 24.3 ms per step.
static bool wide_target(const BqrMat& q, const BqrTarget& t)
{
    const int mode = wide_mode();
    if (mode == 0 || q.k <= NBK || t.kc <= 0) return false;
    if (q.ctl && q.stop_rel2 > 0.0 && t.n_pan < 0) return false; // (skipped panels must be known: their V is never read)
    if (mode == 1) return true;
    return q.k >= kWideMinK && t.kc >= kWideMinKc;
}
// doubles of scratch: the strips' W2 + partials, or the row-chunk partials of one group's W1 (W x kc each)
static size_t scratch_doubles(int64_t m, int64_t n, int64_t kc)
{
    const size_t strips = (size_t)(1 + kWSplit) * NBK * (size_t)std::max<int64_t>(std::max(n, kc), 1);
    const size_t wide = (size_t)w_split(m) * (size_t)wide_width() * (size_t)std::max<int64_t>(kc, 1);
    return std::max(strips, wide);
}

size_t bqr_aux_bytes(int64_t m, int64_t n, int64_t ld, int64_t kc)
{
    const int64_t k = std::min(m, n);
    const int64_t npan = (k + NBK - 1) / NBK;
    return al256(sizeof(double) * (size_t)ld * (size_t)std::max<int64_t>(k, 1)) + al256(sizeof(double) * (size_t)npan * NBK * NBK) +
           al256(sizeof(double) * (size_t)std::max<int64_t>(k, 1)) + al256(sizeof(double) * scratch_doubles(m, n, kc));
}

size_t bqr_carve(BqrMat& q, char* base, int64_t kc)
{
    const int64_t k = q.k;
    const int64_t npan = (k + NBK - 1) / NBK;
    size_t off = 0;
    q.V = reinterpret_cast<double*>(base + off);
    off += al256(sizeof(double) * (size_t)q.ld * (size_t)std::max<int64_t>(k, 1));
    q.T = reinterpret_cast<double*>(base + off);
    off += al256(sizeof(double) * (size_t)npan * NBK * NBK);
    q.tau = reinterpret_cast<double*>(base + off);
    off += al256(sizeof(double) * (size_t)std::max<int64_t>(k, 1));
    q.scratch = reinterpret_cast<double*>(base + off);
    q.scr_half = (int64_t)NBK * std::max<int64_t>(std::max<int64_t>(q.n, kc), 1);
    q.scr_total = (int64_t)scratch_doubles(q.m, q.n, kc);
    off += al256(sizeof(double) * (size_t)q.scr_total);
    return off;
}

// the early-stop fields of a panel descriptor (PanelDesc or PanelDescM, see panel_stop_check)
template <typename Desc>
static void set_panel_stop(Desc& d, const BqrMat& q, int n_parts, int step)
{
    d.ctl = q.ctl;
    d.parts = q.parts;
    d.rel2 = q.stop_rel2;
    d.n_parts = n_parts;
    d.step = step;
}

int bqr_factor(cyb_ctx_t ctx, const std::vector<BqrMat>& mats)
{
    auto pflags = [](const BqrMat& q) { return (q.v_zeroed ? PANEL_V_ZEROED : 0) | (q.reflect_always ? PANEL_REFLECT_ALWAYS : 0); };
    int max_pan = 0;
    for (const auto& q : mats) max_pan = std::max(max_pan, (q.k + NBK - 1) / NBK);
    // A panel step is [panel kernels: one workgroup per matrix (a few for a panel of more than 1536 rows), a latency chain
    // of 32 column steps] -> [trailing update: the 32-column strips of every matrix in one launch, or in two when their rows
    // are split (StripStep)].  Stage 1: the descriptors of a chunk of panel steps (they depend on shapes and pointers only)
    // go into one host image; stage 2: one upload; stage 3: the launches, panel step by panel step.
    struct Step {
        size_t off_pd = 0, off_pdr = 0, off_pdm = 0; // global-memory panels, register-resident panels, multi-workgroup panels
        unsigned n_pd = 0, n_pdr = 0, n_pdm = 0;
        int wave = 0; // every register-resident panel of this step is short enough for the one- / two- / four-wave kernel (1, 2, 4)
        StripStep strips;
    };
    std::vector<Step> steps;
    std::vector<char> image;
    // exchange buffers of the multi-workgroup panel kernel (matrices with more than 1536 rows), one region per matrix:
    // [tickets of all matrices | error word | per matrix: NBK x n_wg x 64 doubles]
    static const bool no_multi = getenv("CYB_QR_NOMULTI") != nullptr;
    static const bool no_reg = getenv("CYB_QR_PANEL_GLOBAL") != nullptr;
    static const bool no_wave = getenv("CYB_QR_NOWAVE") != nullptr;
    std::vector<size_t> x_off(mats.size(), 0);
    size_t x_bytes = 0, n_multi_wg = 0;
    const size_t t_bytes = al256(sizeof(unsigned int) * NBK * mats.size());
    for (size_t qi = 0; qi < mats.size(); ++qi) {
        const int wmax = (mats[qi].m + RPM_ROWS - 1) / RPM_ROWS;
        if (mats[qi].m > RPM_ROWS && std::min(mats[qi].m, mats[qi].n) > 0) {
            x_off[qi] = t_bytes + 256 + x_bytes;
            x_bytes += sizeof(double) * NBK * (size_t)wmax * 64;
            n_multi_wg += (size_t)wmax;
        }
    }
    const bool multi = !no_multi && x_bytes > 0 && n_multi_wg <= (size_t)ctx->n_cu; // (all workgroups of a launch must be resident)
    char* xbase = nullptr;
    if (multi) {
        void* xw = nullptr;
        CYB_TRY(ctx->workspace(al256(t_bytes + 256 + x_bytes), &xw, 3));
        xbase = static_cast<char*>(xw);
        CYB_HIP(hipMemsetAsync(xbase + t_bytes, 0, 256, ctx->stream)); // the error word
    }
    static const bool no_stop = getenv("CYB_QR_NOSTOP") != nullptr;
    auto stoppable = [&](const BqrMat& q) { // (panels of more than 1536 rows stop too when they run on the multi-workgroup kernel)
        return !no_stop && !no_reg && q.ctl && q.parts && q.stop_rel2 > 0.0 && (q.m <= RPM_ROWS || multi);
    };
    size_t n_slots = 0;
    for (const auto& q : mats) n_slots += (size_t)((q.n + NBK - 1) / NBK) * (size_t)bqr_strip_slots(q.m);
    double* wsplit = nullptr;
    CYB_TRY(split_workspace(ctx, n_slots, &wsplit));
    std::vector<int> n_parts_prev(mats.size(), 0); // strips the previous step's update wrote for this matrix
    static const int stop_every = std::max(1, getenv("CYB_QR_STOP_EVERY") ? atoi(getenv("CYB_QR_STOP_EVERY")) : 2);
    for (StepChunks c(max_pan); c.more(); c.next()) {
        steps.clear();
        image.clear();
        for (int p = c.begin; p < c.end; ++p) {
            std::vector<PanelDesc> pd, pd_reg;
            std::vector<PanelDescM> pdm;
            std::vector<StripDesc> sd;
            std::vector<std::pair<int, int>> cnt; // (rows, strips) of every matrix with a trailing block
            for (const auto& q : mats) {
                const int j0 = p * NBK;
                if (j0 >= q.k) continue;
                const int64_t nt = q.n - (j0 + std::min(NBK, q.k - j0));
                if (nt > 0) cnt.push_back({q.m - j0, (int)((nt + NBK - 1) / NBK)});
            }
            const int step_ch = step_chunk_rows(cnt, ctx->n_cu);
            Step st;
            for (size_t qi = 0; qi < mats.size(); ++qi) {
                const auto& q = mats[qi];
                const int j0 = p * NBK;
                if (j0 >= q.k) continue;
                const int pw = std::min(NBK, q.k - j0);
                double* Tp = q.T + (size_t)p * NBK * NBK;
                const bool stop = stoppable(q);
                // ---- the panel: register-resident, spread over several workgroups, or (fallback) in global memory
                if (!no_reg && q.m - j0 <= RPM_ROWS) {
                    pd_reg.push_back(PanelDesc{q.Ac, q.V, Tp, q.tau, q.ld, q.m, j0, pw, pflags(q)});
                    if (stop) set_panel_stop(pd_reg.back(), q, n_parts_prev[qi], p);
                } else if (multi && !no_reg) {
                    const int n_wg = (q.m - j0 + RPM_ROWS - 1) / RPM_ROWS;
                    for (int w = 0; w < n_wg; ++w) {
                        pdm.push_back(PanelDescM{q.Ac, q.V, Tp, q.tau, reinterpret_cast<double*>(xbase + x_off[qi]),
                                                 reinterpret_cast<unsigned int*>(xbase) + qi * NBK, reinterpret_cast<unsigned int*>(xbase + t_bytes),
                                                 q.ld, q.m, j0, pw, pflags(q), w, n_wg, 0, 0});
                        if (stop) set_panel_stop(pdm.back(), q, n_parts_prev[qi], p);
                    }
                } else
                    pd.push_back(PanelDesc{q.Ac, q.V, Tp, q.tau, q.ld, q.m, j0, pw, pflags(q) & PANEL_REFLECT_ALWAYS});
                // ---- the strips of the trailing block A[j0:, j1:]
                const int j1 = j0 + pw;
                const int64_t nt = q.n - j1, mr = q.m - j0;
                n_parts_prev[qi] = 0;
                if (nt <= 0) continue;
                const size_t s_begin = sd.size();
                add_strips(sd, q.Ac + (size_t)j1 * q.ld + j0, q.ld, nt, q.V + (size_t)j0 * q.ld + j0, q.ld, Tp, mr, pw, 1);
                if (stop) {
                    const bool measure = p % stop_every == stop_every - 1; // (the trailing norm is measured every stop_every-th step)
                    const int nch = strip_chunks((int)mr, step_ch); // (every strip of a matrix has the same rows: the same chunks)
                    for (size_t si = s_begin; si < sd.size(); ++si) {
                        sd[si].ctl = q.ctl;
                        sd[si].part_out = measure ? q.parts + (si - s_begin) * (size_t)nch : nullptr;
                        sd[si].step = p;
                    }
                    if (measure) {
                        n_parts_prev[qi] = (int)(sd.size() - s_begin) * nch;
                        st.strips.norm = true;
                    }
                }
            }
            st.n_pd = (unsigned)pd.size();
            st.n_pdr = (unsigned)pd_reg.size();
            st.n_pdm = (unsigned)pdm.size();
            if (st.n_pd) st.off_pd = put(image, pd.data(), sizeof(PanelDesc) * pd.size());
            if (st.n_pdr) st.off_pdr = put(image, pd_reg.data(), sizeof(PanelDesc) * pd_reg.size());
            if (st.n_pdm) st.off_pdm = put(image, pdm.data(), sizeof(PanelDescM) * pdm.size());
            int max_rows = 0;
            for (const auto& d : pd_reg) max_rows = std::max(max_rows, d.m - d.j0);
            st.wave = (no_wave || st.n_pdr == 0) ? 0 : max_rows <= RP_WAVE_ROWS ? 1 : max_rows <= 2 * RP_WAVE_ROWS ? 2 : max_rows <= 4 * RP_WAVE_ROWS ? 4 : 0;
            st.strips.stage(sd, step_ch, wsplit, image);
            steps.push_back(st);
        }
        void* d_image = nullptr;
        CYB_TRY(ctx->upload(image.data(), image.size(), &d_image));
        char* dbase = static_cast<char*>(d_image);
        for (const Step& st : steps) {
            if (st.n_pd)
                hipLaunchKernelGGL(qr_panel_kernel, dim3(st.n_pd), dim3(PNT), 0, ctx->stream,
                                   reinterpret_cast<const PanelDesc*>(dbase + st.off_pd));
            if (st.n_pdm) {
                CYB_HIP(hipMemsetAsync(xbase, 0, t_bytes, ctx->stream)); // the tickets of every matrix
                hipLaunchKernelGGL(qr_panel_multi_kernel, dim3(st.n_pdm), dim3(RP_NT), 0, ctx->stream,
                                   reinterpret_cast<const PanelDescM*>(dbase + st.off_pdm));
            }
            if (st.n_pdr && st.wave == 1)
                hipLaunchKernelGGL(qr_panel_wave_kernel, dim3(st.n_pdr), dim3(64), 0, ctx->stream,
                                   reinterpret_cast<const PanelDesc*>(dbase + st.off_pdr));
            else if (st.n_pdr && st.wave == 2)
                hipLaunchKernelGGL(qr_panel_wave2_kernel, dim3(st.n_pdr), dim3(128), 0, ctx->stream,
                                   reinterpret_cast<const PanelDesc*>(dbase + st.off_pdr));
            else if (st.n_pdr && st.wave == 4)
                hipLaunchKernelGGL(qr_panel_wave4_kernel, dim3(st.n_pdr), dim3(256), 0, ctx->stream,
                                   reinterpret_cast<const PanelDesc*>(dbase + st.off_pdr));
            else if (st.n_pdr)
                hipLaunchKernelGGL(qr_panel_reg_kernel, dim3(st.n_pdr), dim3(RP_NT), 0, ctx->stream,
                                   reinterpret_cast<const PanelDesc*>(dbase + st.off_pdr));
            CYB_HIP(hipGetLastError());
            CYB_TRY(st.strips.launch(ctx, d_image));
        }
    }
    if (multi) { // (the rare path pays one read-back: a poll that ran out of time means wrong factors, not a hang)
        unsigned int h_err = 0;
        CYB_HIP(hipMemcpyAsync(&h_err, xbase + t_bytes, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
        CYB_HIP(hipStreamSynchronize(ctx->stream));
        if (h_err) {
            set_error("blocked QR: a workgroup of the multi-workgroup panel kernel waited more than a second for its partners");
            return CYB_ERR_HIP;
        }
    }
    return CYB_OK;
}

// the strip route of bqr_apply_q: one panel step (32 reflector columns) at a time, last panel first
static int apply_q_strips(cyb_ctx_t ctx, const std::vector<BqrMat>& mats, const std::vector<BqrTarget>& targets)
{
    int max_pan = 0;
    for (const auto& t : targets) max_pan = std::max(max_pan, (mats[(size_t)t.mat].k + NBK - 1) / NBK);
    size_t n_slots = 0;
    for (const auto& t : targets) n_slots += (size_t)((t.kc + NBK - 1) / NBK) * (size_t)bqr_strip_slots(mats[(size_t)t.mat].m);
    double* wsplit = nullptr;
    CYB_TRY(split_workspace(ctx, n_slots, &wsplit));
    std::vector<StripStep> steps;
    std::vector<char> image;
    for (StepChunks c(max_pan); c.more(); c.next()) {
        steps.clear();
        image.clear();
        for (int i = c.begin; i < c.end; ++i) {
            const int p = max_pan - 1 - i;
            std::vector<StripDesc> sd;
            for (const auto& t : targets) {
                const BqrMat& q = mats[(size_t)t.mat];
                const int j0 = p * NBK;
                if (j0 >= q.k || t.kc <= 0) continue;
                CYB_REQUIRE((int64_t)NBK * t.kc <= q.scr_half, "bqr_apply_q: target wider than the carved scratch");
                const size_t s_begin = sd.size();
                // rows j0.. of every column of the target
                add_strips(sd, t.C + j0, t.ldc, t.kc, q.V + (size_t)j0 * q.ld + j0, q.ld, q.T + (size_t)p * NBK * NBK, q.m - j0, std::min(NBK, q.k - j0), 0);
                if (q.ctl && q.stop_rel2 > 0.0) // (panels the factorisation skipped are the identity: their strips return at once)
                    for (size_t si = s_begin; si < sd.size(); ++si) {
                        sd[si].ctl = q.ctl;
                        sd[si].step = p;
                    }
            }
            if (sd.empty()) continue;
            std::vector<std::pair<int, int>> cnt;
            for (const auto& d : sd) cnt.push_back({d.mr, 1});
            StripStep st;
            st.stage(sd, step_chunk_rows(cnt, ctx->n_cu), wsplit, image);
            steps.push_back(st);
        }
        if (steps.empty()) continue;
        void* d_image = nullptr;
        CYB_TRY(ctx->upload(image.data(), image.size(), &d_image));
        for (const auto& st : steps) CYB_TRY(st.launch(ctx, d_image));
    }
    return CYB_OK;
}

// The wide route of bqr_apply_q.  Nothing between two panel steps of an application depends on a factorisation, so the
// reflectors are applied in groups of W = CYB_QR_APPLY_WIDTH columns, last group first:
//   once per call, off the chain of C:  Gram blocks of every group (one grouped-GEMM launch) -> merged factors T_S
//   (merge_t_kernel) -> VT_S = V_S T_S (one grouped-GEMM launch);
//   per group, for the whole batch:     W1 = V_S^T C[j0_S:, :] in row chunks (w_split: the narrow output fills the chip), the
//   partials summed in a fixed order (sum_partials_kernel), then C[j0_S:, :] -= VT_S W1.
// C is streamed once per W reflector columns instead of once per 32, and both products have the shape of an ordinary GEMM.
static int apply_q_wide(cyb_ctx_t ctx, const std::vector<BqrMat>& mats, const std::vector<BqrTarget>& targets)
{
    const int W = wide_width();
    struct Tgt {
        const BqrMat* q;
        const BqrTarget* t;
        int k_eff, ng; // reflector columns that are applied (the panels behind an early stop are the identity), groups
        double* VT;    // V_S T_S of every group, laid out like V (element (i, c) at c * ld + i)
        double* TS;    // ng images of W x W
        double* G;     // Gram partials: per group n_gp images of W x W
        std::vector<int> n_gp;
    };
    std::vector<Tgt> tg;
    size_t bytes = 0;
    int max_ng = 0;
    for (const auto& t : targets) {
        const BqrMat& q = mats[(size_t)t.mat];
        const int npan = (q.k + NBK - 1) / NBK;
        const int nf = t.n_pan >= 0 ? std::min(npan, (int)t.n_pan) : npan;
        const int k_eff = std::min<int>(q.k, nf * NBK);
        if (k_eff <= 0 || t.kc <= 0) continue;
        Tgt g{&q, &t, k_eff, (k_eff + W - 1) / W, nullptr, nullptr, nullptr, {}};
        CYB_REQUIRE((int64_t)w_split(q.m) * W * t.kc <= q.scr_total, "bqr_apply_q: target wider than the carved scratch");
        for (int s = 0; s < g.ng; ++s) {
            // row chunks of the group's Gram blocks: every block column keeps at least 256 rows per chunk
            const int j0 = s * W, w = std::min(W, k_eff - j0);
            const int min_rows = q.m - j0 - (w - 1) / NBK * NBK;
            g.n_gp.push_back(std::max(1, std::min(4, min_rows / 256)));
        }
        max_ng = std::max(max_ng, g.ng);
        tg.push_back(std::move(g));
    }
    if (tg.empty()) return CYB_OK;
    std::vector<size_t> o_vt(tg.size()), o_ts(tg.size()), o_g(tg.size());
    for (size_t i = 0; i < tg.size(); ++i) {
        size_t n_g = 0;
        for (int n : tg[i].n_gp) n_g += (size_t)n;
        o_vt[i] = bytes;
        bytes += al256(sizeof(double) * (size_t)tg[i].q->ld * (size_t)tg[i].k_eff);
        o_ts[i] = bytes;
        bytes += al256(sizeof(double) * (size_t)tg[i].ng * W * W);
        o_g[i] = bytes;
        bytes += al256(sizeof(double) * n_g * W * W);
    }
    void* ws = nullptr;
    CYB_TRY(ctx->workspace(bytes, &ws, 5));
    for (size_t i = 0; i < tg.size(); ++i) {
        tg[i].VT = reinterpret_cast<double*>(static_cast<char*>(ws) + o_vt[i]);
        tg[i].TS = reinterpret_cast<double*>(static_cast<char*>(ws) + o_ts[i]);
        tg[i].G = reinterpret_cast<double*>(static_cast<char*>(ws) + o_g[i]);
    }
    std::vector<char> image;
    // ---- merged factors of every group of every target
    {
        GemmBatch gg, gv;
        std::vector<MergeDesc> md;
        for (const Tgt& g : tg) {
            const BqrMat& q = *g.q;
            size_t gp0 = 0;
            for (int s = 0; s < g.ng; ++s) {
                const int j0 = s * W, w = std::min(W, g.k_eff - j0), n_gp = g.n_gp[(size_t)s];
                const double* Vs = q.V + (size_t)j0 * q.ld + j0; // V_S: element (i, a) at a * ld + i, i < m - j0
                double* Gs = g.G + gp0 * (size_t)W * W;
                double* TSs = g.TS + (size_t)s * W * W;
                for (int a = NBK; a < w; a += NBK) {
                    // G[0:a, a:a+wb] = V_S[a:, 0:a]^T V_S[a:, a:a+wb]  (the columns from a on are zero above row a)
                    const int wb = std::min(NBK, w - a);
                    const int64_t rows = q.m - j0 - a, chunk = (rows + n_gp - 1) / n_gp;
                    for (int p = 0; p < n_gp; ++p) {
                        const int64_t r0 = a + chunk * p, kr = std::min(chunk, rows - chunk * p);
                        gg.add(Gs + (size_t)p * W * W + a, a, wb, W, Vs + r0, q.ld, 1, Vs + (size_t)a * q.ld + r0, 1, q.ld, kr, 1.0, 0.0);
                    }
                }
                md.push_back(MergeDesc{Gs, q.T + (size_t)(j0 / NBK) * NBK * NBK, TSs, (int64_t)W * W, w, W, n_gp, 0});
                // VT_S^T (w x rows, row stride ld) = T_S^T V_S^T
                gv.add(g.VT + (size_t)j0 * q.ld + j0, w, q.m - j0, q.ld, TSs, 1, W, Vs, q.ld, 1, w, 1.0, 0.0);
                gp0 += (size_t)n_gp;
            }
        }
        GemmStaged sg, sv;
        CYB_TRY(gg.stage(ctx, image, sg));
        CYB_TRY(gv.stage(ctx, image, sv));
        const size_t off_md = (image.size() + 255) / 256 * 256;
        image.resize(off_md + sizeof(MergeDesc) * md.size());
        memcpy(image.data() + off_md, md.data(), sizeof(MergeDesc) * md.size());
        void* d_image = nullptr;
        CYB_TRY(ctx->upload(image.data(), image.size(), &d_image));
        CYB_TRY(gemm_launch_staged(ctx, sg, d_image));
        const MergeDesc* mdp = reinterpret_cast<const MergeDesc*>(static_cast<char*>(d_image) + off_md);
        if (W <= 128) hipLaunchKernelGGL(merge_t_kernel<96>, dim3((unsigned)md.size()), dim3(MG_NT), 0, ctx->stream, mdp);
        else hipLaunchKernelGGL(merge_t_kernel<224>, dim3((unsigned)md.size()), dim3(MG_NT), 0, ctx->stream, mdp);
        CYB_HIP(hipGetLastError());
        CYB_TRY(gemm_launch_staged(ctx, sv, d_image));
    }
    // ---- the groups, last first, staged in growing chunks (2, 6, 18, ... groups): the host lays out the next chunk while
    //      the device runs the previous ones
    struct Step {
        GemmStaged s1, s2;
        size_t off_sum = 0;
        unsigned n_sum = 0;
    };
    std::vector<Step> steps;
    int chunk = 2;
    for (int c0 = max_ng - 1; c0 >= 0; c0 -= chunk, chunk *= 3) {
        const int c1 = std::max(-1, c0 - chunk);
        steps.clear();
        image.clear();
        for (int s = c0; s > c1; --s) {
            GemmBatch g1, g2;
            std::vector<SumDesc> sums;
            for (const Tgt& g : tg) {
                if (s >= g.ng) continue;
                const BqrMat& q = *g.q;
                const BqrTarget& t = *g.t;
                const int j0 = s * W, w = std::min(W, g.k_eff - j0);
                const int64_t mr = q.m - j0;
                const double* Vs = q.V + (size_t)j0 * q.ld + j0;
                const double* VTs = g.VT + (size_t)j0 * q.ld + j0;
                double* Ct = t.C + j0; // rows j0.. of every column
                const int ns = w_split(mr);
                const int64_t rch = ((mr + ns - 1) / ns + 15) / 16 * 16;
                const int64_t stride = (int64_t)W * t.kc;
                int n_part = 0;
                for (int sidx = 0; sidx < ns; ++sidx) {
                    const int64_t r0 = rch * sidx, rows = std::min(rch, mr - r0);
                    if (rows <= 0) break;
                    // partial W1 (w x kc row-major) of this row chunk
                    g1.add(q.scratch + (size_t)sidx * (size_t)stride, w, t.kc, t.kc, Vs + r0, q.ld, 1, Ct + r0, 1, t.ldc, rows, 1.0, 0.0);
                    ++n_part;
                }
                if (n_part > 1) sums.push_back(SumDesc{q.scratch, (int64_t)w * t.kc, stride, n_part, 0});
                // C^T (kc x mr, row stride ldc) -= W1^T VT_S^T
                g2.add(Ct, t.kc, mr, t.ldc, q.scratch, 1, t.kc, VTs, q.ld, 1, w, -1.0, 1.0);
            }
            if (g1.empty()) continue;
            Step st;
            CYB_TRY(g1.stage(ctx, image, st.s1));
            CYB_TRY(g2.stage(ctx, image, st.s2));
            if (!sums.empty()) {
                st.n_sum = (unsigned)sums.size();
                st.off_sum = (image.size() + 255) / 256 * 256;
                image.resize(st.off_sum + sizeof(SumDesc) * sums.size());
                memcpy(image.data() + st.off_sum, sums.data(), sizeof(SumDesc) * sums.size());
            }
            steps.push_back(st);
        }
        if (steps.empty()) continue;
        void* d_image = nullptr;
        CYB_TRY(ctx->upload(image.data(), image.size(), &d_image));
        for (const auto& st : steps) {
            CYB_TRY(gemm_launch_staged(ctx, st.s1, d_image));
            if (st.n_sum) {
                hipLaunchKernelGGL(sum_partials_kernel, dim3(helper_grid_x(st.n_sum), st.n_sum), dim3(256), 0, ctx->stream,
                                   reinterpret_cast<const SumDesc*>(static_cast<char*>(d_image) + st.off_sum));
                CYB_HIP(hipGetLastError());
            }
            CYB_TRY(gemm_launch_staged(ctx, st.s2, d_image));
        }
    }
    return CYB_OK;
}

// the route of every target of ONE application (targets[begin : end]): see wide_target
static void split_routes(const std::vector<BqrMat>& mats, const std::vector<BqrTarget>& targets, size_t begin, size_t end,
                         std::vector<BqrTarget>& narrow, std::vector<BqrTarget>& wide)
{
    const size_t w0 = wide.size();
    int64_t cols = 0;
    for (size_t i = begin; i < end; ++i) {
        const BqrTarget& t = targets[i];
        if (wide_target(mats[(size_t)t.mat], t)) {
            wide.push_back(t);
            cols += t.kc;
        } else narrow.push_back(t);
    }
    if (wide_mode() < 0 && cols < kWideMinCols) { // (see wide_target)
        wide.resize(w0);
        narrow.assign(targets.begin() + (std::ptrdiff_t)begin, targets.begin() + (std::ptrdiff_t)end);
    }
    static const bool trace = getenv("CYB_QR_TRACE_ROUTE") != nullptr; // (test hook: the route every application took)
    if (trace)
        fprintf(stderr, "[cyb] apply_q: %zu targets, %zu wide (%lld columns qualify), %zu on strips\n", end - begin, wide.size() - w0,
                (long long)cols, narrow.size());
}

int bqr_apply_q(cyb_ctx_t ctx, const std::vector<BqrMat>& mats, const std::vector<BqrTarget>& targets)
{
    // the two routes work on disjoint targets (and on the scratch of disjoint matrices)
    std::vector<BqrTarget> narrow, wide;
    split_routes(mats, targets, 0, targets.size(), narrow, wide);
    if (!narrow.empty()) CYB_TRY(apply_q_strips(ctx, mats, narrow));
    if (!wide.empty()) CYB_TRY(apply_q_wide(ctx, mats, wide));
    return CYB_OK;
}

int bqr_apply_q_pair(cyb_ctx_t ctx, const std::vector<BqrMat>& mats, const std::vector<BqrTarget>& targets, size_t n_first)
{
    n_first = std::min(n_first, targets.size());
    std::vector<BqrTarget> narrow_a, narrow_b, wide;
    split_routes(mats, targets, 0, n_first, narrow_a, wide);
    split_routes(mats, targets, n_first, targets.size(), narrow_b, wide);
    if (!narrow_a.empty()) CYB_TRY(apply_q_strips(ctx, mats, narrow_a));
    if (!narrow_b.empty()) CYB_TRY(apply_q_strips(ctx, mats, narrow_b));
    if (!wide.empty()) CYB_TRY(apply_q_wide(ctx, mats, wide));
    return CYB_OK;
}

} // namespace cyb
