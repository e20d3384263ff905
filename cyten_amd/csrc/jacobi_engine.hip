// One-sided block-Jacobi orthogonalisation on gfx950 (engine of the batched SVD / eigh).
//
// Replaces the per-block LAPACK calls of the reference (scipy.linalg.svd -> dgesdd,
// src/block_backend/numpy.cpp:1247-1297; np.linalg.eigh -> dsyevd, numpy.cpp:658-680) with a
// Hestenes one-sided Jacobi in *block* form so that the O(len * nv^2) work per sweep runs on the
// f64 MFMA pipe.  The rows of a matrix are cut into blocks of JB=16 vectors; a sweep takes every pair of blocks
// (P,Q) once, in the nb - 1 rounds of a round-robin schedule.  A pair visit is
//     Gram   G = X X^T       X = [W_P; W_Q] (32 x len), MFMA 16x16x4 f64 straight from global memory
//     eigh   G ~ Qm L Qm^T   two-sided Jacobi on the 32x32 Gram matrix in LDS, deflation of numerically null
//                            rows, in-pair descending sort
//     update X <- Qm^T X     on W, and on J where the rotations are accumulated (64-column chunks, MFMA)
// and the per-sweep convergence measure max |g_ij|/sqrt(g_ii g_jj) is accumulated with an atomic max.
//
// THE ENGINE is the persistent sweep, jacobi_sweep_kernel: ONE launch per sweep (or for all sweeps of a list of small
// matrices), every (pair slot, column part) workgroup resident for the whole launch, rounds handed on through counters
// in memory.  Its plan -- parts per pair, shared workgroups, layout of the counters, convergence rule -- is
// jacobi_plan.h.  The host reads the off-norms once per sweep.
//
// THE FALLBACK is the split route, jacobi_gram_kernel + jacobi_update_kernel: two launches per round, no residency
// constraint, operands addressed with 64-bit pointers.  It serves lists that hold a matrix of 2^31 bytes or more (the
// sweep kernel addresses W and J through 32-bit buffer offsets) and CYB_JACOBI_NOSWEEP, the test hook that keeps it
// exercised; embedded complex rows have no fallback and are refused there.
#include "jacobi_engine.h"
#include "jacobi_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace cyb {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
#define GLOBAL_AS __attribute__((address_space(1)))
typedef const GLOBAL_AS d2* gc2;
typedef const GLOBAL_AS d2* gcp2;
typedef GLOBAL_AS double* gp;

constexpr int GS = JP + 2;   // row stride of the Gram matrix in LDS
constexpr int QS = JP + 16;  // row stride of Qm in LDS ([k][m] layout: 48 = 16 mod 32 -> conflict-free)
constexpr int GK = 64;       // k extent of one Gram staging tile
constexpr int XS = GK + 2;   // its row stride ([m][k] layout)
constexpr int NT = 256;
constexpr int NPAIR = JP / 2;
static_assert(JP == 32, "the wave tiling below assumes 32 x 32 pair problems");

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// max over the workgroup; `red` is 8 doubles of LDS. All threads get the result.
__device__ __forceinline__ double block_max(double v, double* red, int tid)
{
    v = wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// scaled off-diagonal measure of the JP x JP Gram matrix in LDS
__device__ __forceinline__ double gram_offmax(const double* Gs, double* red, int tid)
{
    double m = 0.0;
#pragma unroll
    for (int e = tid; e < JP * JP; e += NT) {
        const int i = e / JP, j = e % JP;
        if (i < j) {
            const double den = Gs[i * GS + i] * Gs[j * GS + j];
            if (den > 0.0) m = fmax(m, fabs(Gs[i * GS + j]) * rsqrt(den));
        }
    }
    return block_max(m, red, tid);
}

// pair of players meeting in round r (0..n-2), slot k (0..n/2-1) of the circle method, n even
__host__ __device__ __forceinline__ void circle_pair(int n, int r, int k, int& p, int& q)
{
    const int m = n - 1;
    if (k == 0) {
        p = m;
        q = r;
    } else {
        p = r + k;
        if (p >= m) p -= m;
        q = r - k;
        if (q < 0) q += m;
    }
}

// v_rsq_f64 refined with two Newton steps (full double precision for the rotation)
__device__ __forceinline__ double fast_rsqrt(double x)
{
    double r = __builtin_amdgcn_rsq(x);
    r = r * (1.5 - 0.5 * x * r * r);
    r = r * (1.5 - 0.5 * x * r * r);
    return r;
}

// Symmetric 2x2 Jacobi rotation [[c, s], [-s, c]] that annihilates b in [[a, b], [b, d]] (the small
// angle |theta| <= pi/4).  Division-free: with delta = d - a, h = hypot(delta, 2b):
//   cos 2theta = |delta| / h,  c = sqrt((1 + cos 2theta) / 2),  s = sign(delta b) |b| / (h c).
// Two v_rsq_f64 + a dozen FMAs instead of two IEEE divisions and two square roots: the inner
// eigensolver runs one wave per SIMD, so every dependent long-latency op is exposed.
// thr2: relative threshold, as in jacobi_rot_bf below -- a coupling with b^2 <= thr2 a d is left alone.
__device__ __forceinline__ void jacobi_rot(double a, double d, double b, double& c, double& s, double thr2 = 0.0)
{
    const double delta = d - a;
    const double h2 = delta * delta + 4.0 * b * b;
    c = 1.0;
    s = 0.0;
    if (fabs(b) > 1e-300 && h2 > 1e-300 && b * b > thr2 * a * d) {
        const double rh = fast_rsqrt(h2);            // 1 / h
        const double c2 = 0.5 + 0.5 * fabs(delta) * rh; // cos^2 theta in [1/2, 1]
        const double rc = fast_rsqrt(c2);            // 1 / c
        c = c2 * rc;
        const double sg = ((delta >= 0.0) == (b >= 0.0)) ? 1.0 : -1.0;
        s = sg * fabs(b) * rh * rc;
    }
}

__device__ __forceinline__ int xrow(int i, int P, int Q) { return (i < JB) ? P * JB + i : Q * JB + (i - JB); }

// ================================================================================================
// Split route (the fallback): TWO launches per round of the round-robin schedule.
//
// Per-round scratch shared by the two kernels of a round (one entry per block pair of the round).
struct JScratch {
    double* gpart;        // [pair][part][JP*JP]  partial Gram matrices
    // the three result arrays of a round exist twice (index = round parity): the J half of a round's
    // update is applied one launch later, beside the next round's Gram/eigensolve
    double* qout[2];      // [pair][JP*JP]        Qm as [k][m], output-row order
    int32_t* zout[2];     // [pair][JP]           1: output row is deflated (write zeros)
    int32_t* flag[2];     // [pair]               1: apply the update, 0: pair already orthogonal
    unsigned int* cnt;    // [pair]               arrival counter of the Gram parts (self-resetting)
};

// Kernel A of a round.  grid = pairs x G.  Every workgroup computes the Gram partial of its K range;
// the last of the G parts of a pair to arrive (write-through stores, drained, one atomic ticket,
// L1-bypassing loads: cdna_hip_programming.md Guideline 16) sums the partials in a FIXED order, then does the
// deflation test, the convergence measure and the two-sided Jacobi eigh of the 32x32 Gram in LDS,
// and publishes Qm for kernel B.  No workgroup ever waits for another one.
__device__ __forceinline__ void update_role(const JMat* __restrict__ mats, const JWork* __restrict__ work, int round,
                                            int pi, int unit, int U, const JScratch& sc, int buf, bool do_w, bool do_j,
                                            double* smem, int* zflag);

// Workgroups beyond the first n_gram of the grid take the update role for the J half of the PREVIOUS
// round (prev_round, hand-off buffer buf ^ 1): nothing reads J before the end, so that half of the
// update leaves the critical path and runs beside this round's Gram / eigensolve.
__global__ void __launch_bounds__(NT, 2)
jacobi_gram_kernel(const JMat* __restrict__ mats, const JWork* __restrict__ work, int round, int G, int max_inner,
                   unsigned long long* __restrict__ offmax_bits, JScratch sc, int buf, int n_gram, int prev_round, int UJ)
{
    constexpr int STAGE = 2 * JP * XS > 4 * JP * GS ? 2 * JP * XS : 4 * JP * GS;
    __shared__ __attribute__((aligned(16))) double smem[2 * JP * GS + JP * QS + STAGE + 8];
    __shared__ int perm[JP];   // output row -> eigenvector column (descending eigenvalue)
    __shared__ int zrow[JP];   // 1: this row of the pair is numerically null (deflated)
    __shared__ int s_any_null, s_last;
    __shared__ unsigned short sched[(JP - 1) * NPAIR];
    double* Gs = smem;
    double* G2 = Gs + JP * GS;
    double* Qs = G2 + JP * GS;
    double* Xc = Qs + JP * QS;
    double* red = Xc + STAGE;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= n_gram) {
        const int b = (int)blockIdx.x - n_gram;
        update_role(mats, work, prev_round, b / UJ, b % UJ, UJ, sc, buf ^ 1, false, true, smem, zrow);
        return;
    }
    const int pi = blockIdx.x / G, part = blockIdx.x % G;

    const JWork wk = work[pi];
    const JMat mt = mats[wk.mat];
    if (round >= mt.nb - 1) return; // this matrix has fewer rounds per sweep
    int P, Q;
    circle_pair(mt.nb, round, wk.slot, P, Q);
    if (P > Q) {
        const int t = P;
        P = Q;
        Q = t;
    }

    // ---- 1. partial Gram over this part's share of K
    {
        gp W = (gp)mt.W;
        const int ld = mt.lenp;
        d4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
        // Operands go from global memory straight into the MFMA: lane (r = lane & 15, g = lane >> 4)
        // loads the two doubles X[r][k0 + 2g], X[r][k0 + 2g + 1] of rows r and r + 16 (16-byte loads,
        // 64 contiguous bytes per row and wave) and feeds .x to one MFMA k-step and .y to the next --
        // both operands of a Gram product are the same matrix, so any pairing of k positions that is
        // the same for the two of them is right.  No staging tile, no barrier in the loop; the four
        // waves take the 8-deep k chunks round-robin.
        const int r = lane & 15, g2 = 2 * (lane >> 4);
        gcp2 s0 = (gcp2)(W + (int64_t)xrow(r, P, Q) * ld + g2);
        gcp2 s1 = (gcp2)(W + (int64_t)xrow(r + 16, P, Q) * ld + g2);
        const int nchunk_all = ld / 8; // ld is a multiple of 64 (zero padded)
        const int c_begin = (int)((int64_t)part * nchunk_all / G), c_end = (int)((int64_t)(part + 1) * nchunk_all / G);
        // the loop is bound by load latency (the rows were written by the previous launch): UN chunks
        // per wave are in flight while the previous UN are multiplied
        constexpr int UN = 8;
        d2 x0[UN], x1[UN], n0[UN], n1[UN];
        auto load = [&](d2 (&a0)[UN], d2 (&a1)[UN], int c0) {
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int c = min(c0 + 4 * u, c_end - 1); // clamped: a duplicate is masked out in the product
                a0[u] = s0[c * 4];
                a1[u] = s1[c * 4];
            }
        };
        if (c_begin + wave < c_end) load(x0, x1, c_begin + wave);
        for (int c0 = c_begin + wave; c0 < c_end; c0 += 4 * UN) {
            const bool more = c0 + 4 * UN < c_end; // wave-uniform
            if (more) load(n0, n1, c0 + 4 * UN);
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                if (c0 + 4 * u < c_end) { // wave-uniform
                    // the (1,0) tile is the transpose of (0,1): not computed (the phase is bound by
                    // the MFMA pipe of the one or two CUs that work on a pair)
                    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u].x, x0[u].x, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u].x, x1[u].x, acc[0][1], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u].x, x1[u].x, acc[1][1], 0, 0, 0);
                    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u].y, x0[u].y, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u].y, x1[u].y, acc[0][1], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u].y, x1[u].y, acc[1][1], 0, 0, 0);
                }
            }
            if (more) {
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    x0[u] = n0[u];
                    x1[u] = n1[u];
                }
            }
        }
        double* wpart = Xc + wave * (JP * GS);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (i == 1 && j == 0) // mirror of tile (0,1)
                        wpart[(16 + (lane & 15)) * GS + (lane >> 4) + 4 * r] = acc[0][1][r];
                    else
                        wpart[(i * 16 + (lane >> 4) + 4 * r) * GS + j * 16 + (lane & 15)] = acc[i][j][r];
                }
    }
    __syncthreads();
    if (G == 1) {
        // sum the four wave slices and symmetrise, straight into Gs
        for (int e = tid; e < JP * JP; e += NT) {
            const int i = e / JP, j = e % JP;
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < 4; ++w) s += Xc[w * (JP * GS) + i * GS + j];
            Gs[i * GS + j] = s;
        }
        __syncthreads();
    } else {
        // publish this part's Gram partial (sum over the wave slices), then take a ticket
        GLOBAL_AS double* mine = (GLOBAL_AS double*)(sc.gpart + ((size_t)pi * G + part) * (JP * JP));
        for (int e = tid; e < JP * JP; e += NT) {
            const int i = e / JP, j = e % JP;
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < 4; ++w) s += Xc[w * (JP * GS) + i * GS + j];
            // EVERY store of the handed-off bytes is an 8-byte agent-scope (write-through, sc1) store ...
            __hip_atomic_store((double*)(mine + e), s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // ... drained by every storing wave ...
        __syncthreads();                                  // ... before ONE lane takes the ticket
        if (tid == 0) {
            const unsigned int old = __hip_atomic_fetch_add(sc.cnt + pi, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (old == (unsigned int)(G - 1)) ? 1 : 0;
            if (s_last) __hip_atomic_store(sc.cnt + pi, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // re-arm
        }
        __syncthreads();
        if (!s_last) return;
        // the last arriver reads every partial with agent-scope (sc1, L1-bypassing) loads: no fence needed
        // (MI355X_MICROARCH.md, valid hand-off forms: sc1 stores + drained counter add + sc1 loads)
        const GLOBAL_AS double* all = (const GLOBAL_AS double*)(sc.gpart + (size_t)pi * G * (JP * JP));
        for (int e = tid; e < JP * JP; e += NT) {
            const int i = e / JP, j = e % JP;
            double s = 0.0;
            // (every partial is exactly symmetric: the diagonal tiles are X X^T products accumulated in
            //  the same order on both sides of the diagonal, the (1,0) tile is a copy of (0,1))
            for (int g = 0; g < G; ++g)
                s += __hip_atomic_load((double*)(all + (size_t)g * (JP * JP) + i * JP + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            Gs[i * GS + j] = s;
        }
        __syncthreads();
    }
    // ---- 2a. deflation: rows whose squared norm fell below the numerical-rank threshold are
    //          removed from the problem (zeroed); they are completed after convergence.
    if (tid == 0) s_any_null = 0;
    __syncthreads();
    if (tid < JP) {
        const double thr2 = mt.thr2;
        const double g = Gs[tid * GS + tid];
        const int z = (g > 0.0 && g <= thr2) ? 1 : 0;
        zrow[tid] = z;
        perm[tid] = tid;
        if (z) s_any_null = 1;
    }
    __syncthreads();
    const bool any_null = s_any_null != 0;
    if (any_null) {
        for (int e = tid; e < JP * JP; e += NT) {
            const int i = e / JP, j = e % JP;
            if (zrow[i] || zrow[j]) Gs[i * GS + j] = 0.0;
        }
        __syncthreads();
    }
    // ---- 2b. convergence measure; nothing to do if this pair is already orthogonal --------
    double off = gram_offmax(Gs, red, tid);
    if (tid == 0) {
        atomicMax(offmax_bits + wk.mat, (unsigned long long)__double_as_longlong(off));
        sc.flag[buf][pi] = (off <= mt.tol && !any_null) ? 0 : 1;
    }
    if (off <= mt.tol && !any_null) return;

    // ---- 3. two-sided Jacobi eigh of G in LDS, Qm accumulated ----------------------------
    for (int e = tid; e < JP * QS; e += NT) Qs[e] = ((e / QS) == (e % QS)) ? 1.0 : 0.0;
    for (int e = tid; e < (JP - 1) * NPAIR; e += NT) { // round-robin schedule (circle method) as a table
        int p, q;
        circle_pair(JP, e / NPAIR, e % NPAIR, p, q);
        sched[e] = (unsigned short)(p | (q << 8));
    }
    __syncthreads();
    // One barrier per round: G is double buffered (read Ga, write Gb).  The eigensolver runs one wave
    // per SIMD, so it is bound by the instruction count per round: every thread derives ONE rotation
    // itself (its column pair pc; 16 lanes compute the same one instead of waiting for a publish
    // through LDS) and takes the rotation of its row pair pr from the lane of its 16-lane group that
    // has pc == pr; the pair indices come from the table.
    double* Ga = Gs;
    double* Gb = G2;
    for (int sweep = 0; sweep < (off <= mt.tol ? 0 : max_inner); ++sweep) {
        for (int r = 0; r < JP - 1; ++r) {
            const int pr = tid >> 4, pc = tid & 15;
            const unsigned int sr = sched[r * NPAIR + pr], scl = sched[r * NPAIR + pc];
            const int i = sr & 255, j = sr >> 8, k = scl & 255, l = scl >> 8;
            double c2, s2;
            // (tol / 2)^2: two rows of equal norm are not turned by 45 degrees on a coupling of rounding noise.  eigh iterates
            // on A + shift, every row norm within a factor three of the next and the null space of A one exact cluster: without the
            // threshold those turns went on sweep after sweep and left 1.4e-13 ... 2.2e-13 ||A||_F in the eigenvalues of a
            // 128 / 256-row block with a null space of half its rows (tests/test_gpu_decomp_accuracy.py, variant per-round)
            jacobi_rot(Ga[k * GS + k], Ga[l * GS + l], Ga[k * GS + l], c2, s2, 0.25 * mt.tol * mt.tol);
            const int srcl = (lane & 48) | pr;
            const double c1 = __shfl(c2, srcl), s1 = __shfl(s2, srcl);
            {   // G <- R^T G R on one 2x2 sub-block per thread: rows (i,j), cols (k,l)
                const double gik = Ga[i * GS + k], gil = Ga[i * GS + l];
                const double gjk = Ga[j * GS + k], gjl = Ga[j * GS + l];
                const double hik = c1 * gik - s1 * gjk, hil = c1 * gil - s1 * gjl;
                const double hjk = s1 * gik + c1 * gjk, hjl = s1 * gil + c1 * gjl;
                double nik = c2 * hik - s2 * hil, nil = s2 * hik + c2 * hil;
                double njk = c2 * hjk - s2 * hjl, njl = s2 * hjk + c2 * hjl;
                if (pr == pc) { // the rotated 2x2 diagonal block is diagonal by construction
                    nil = 0.0;
                    njk = 0.0;
                }
                Gb[i * GS + k] = nik;
                Gb[i * GS + l] = nil;
                Gb[j * GS + k] = njk;
                Gb[j * GS + l] = njl;
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) { // Qm <- Qm R : columns (k,l) of rows (tid>>4) and (tid>>4)+16
                const int row = (tid >> 4) + 16 * t;
                const double qk = Qs[row * QS + k], ql = Qs[row * QS + l];
                Qs[row * QS + k] = c2 * qk - s2 * ql;
                Qs[row * QS + l] = s2 * qk + c2 * ql;
            }
            __syncthreads();
            double* tsw = Ga;
            Ga = Gb;
            Gb = tsw;
        }
        if (sweep + 1 < max_inner) { // (no test after the last sweep: two barriers for nothing)
            const double off_in = gram_offmax(Ga, red, tid);
            if (off_in <= 0.25 * mt.tol) break;
        }
    }
    __syncthreads();
    // de Rijk-style ordering inside the pair: larger norms to the lower rows (fewer sweeps)
    if (off > mt.tol && tid < JP) {
        // padding vectors (index >= nv: zero rows of W, identity rows of J) must stay behind the real
        // ones whatever the rounding of the rotated diagonal says: a real row whose eigenvalue came out as
        // -1e-16 would otherwise trade places with a padding row and leave the first nv rows for good
        // (exactly rank-deficient inputs: an all-ones block lost two rows of its accumulated factor)
        auto key = [&](int i) { return xrow(i, P, Q) < mt.nv ? Ga[i * GS + i] : -1.0e300; };
        const double g = key(tid);
        int rk = 0;
        for (int j = 0; j < JP; ++j) {
            const double gj = key(j);
            rk += (gj > g || (gj == g && j < tid)) ? 1 : 0;
        }
        perm[rk] = tid;
    }
    __syncthreads();
    // ---- 4. publish Qm in output-row order (column perm[r] of Qm feeds output row r) -----
    GLOBAL_AS double* qo = (GLOBAL_AS double*)(sc.qout[buf] + (size_t)pi * (JP * JP));
    for (int e = tid; e < JP * JP; e += NT) {
        const int k = e / JP, r = e % JP;
        qo[e] = Qs[k * QS + perm[r]];
    }
    if (tid < JP) sc.zout[buf][(size_t)pi * JP + tid] = zrow[perm[tid]];
}

// Update role: unit `unit` of U of pair `pi` applies X <- Qm^T X to its share of the 64-column chunks
// of W (do_w) and / or J (do_j), with the round's result taken from hand-off buffer `buf`.
// `smem` needs JP*QS doubles, `zflag` JP ints.
// The rows go from global memory straight into the MFMA B operand (lane (n = lane & 15, kq = lane >> 4)
// loads X[4 kk + kq][16 wave + n], 128 contiguous bytes per row and load) and the result straight back:
// each wave owns 16 columns of a chunk, so nothing is staged in LDS, there is no barrier in the loop, and
// the first chunk's loads are in flight while Qm is still being fetched.
__device__ __forceinline__ void update_role(const JMat* __restrict__ mats, const JWork* __restrict__ work, int round,
                                            int pi, int unit, int U, const JScratch& sc, int buf, bool do_w, bool do_j,
                                            double* smem, int* zflag)
{
    double* Qs = smem;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const JWork wk = work[pi];
    const JMat mt = mats[wk.mat];
    if (round >= mt.nb - 1) return;
    if (sc.flag[buf][pi] == 0) return; // pair already orthogonal
    int P, Q;
    circle_pair(mt.nb, round, wk.slot, P, Q);
    if (P > Q) {
        const int t = P;
        P = Q;
        Q = t;
    }
    const int cw = do_w ? mt.lenp / 64 : 0, cj = (do_j && mt.J) ? mt.nvp / 64 : 0;
    const int ct = cw + cj;
    const int c_begin = (int)((int64_t)unit * ct / U), c_end = (int)((int64_t)(unit + 1) * ct / U);
    if (c_begin >= c_end) return;
    // operand pointer of chunk c (the unit's range may straddle the W | J boundary)
    const int n = lane & 15, kq = lane >> 4;
    auto chunk_ptr = [&](int c, int k) -> gp {
        const bool in_w = c < cw;
        gp base = (gp)(in_w ? mt.W : mt.J);
        const int ld = in_w ? mt.lenp : mt.nvp;
        const int cc = in_w ? c : c - cw;
        return base + (int64_t)xrow(k, P, Q) * ld + cc * 64 + wave * 16 + n;
    };
    double xb[JP / 4], xn[JP / 4];
#pragma unroll
    for (int kk = 0; kk < JP / 4; ++kk) xb[kk] = *chunk_ptr(c_begin, 4 * kk + kq);
    const GLOBAL_AS double* qo = (const GLOBAL_AS double*)(sc.qout[buf] + (size_t)pi * (JP * JP));
    for (int e = tid; e < JP * JP; e += NT) Qs[(e / JP) * QS + (e % JP)] = qo[e];
    if (tid < JP) zflag[tid] = sc.zout[buf][(size_t)pi * JP + tid];
    __syncthreads();
    const double* ap0 = Qs + (lane >> 4) * QS + (lane & 15);
    const double* ap1 = ap0 + 16;
    int zr[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) zr[i][r] = zflag[i * 16 + (lane >> 4) + 4 * r];
    for (int c = c_begin; c < c_end; ++c) {
        if (c + 1 < c_end) {
#pragma unroll
            for (int kk = 0; kk < JP / 4; ++kk) xn[kk] = *chunk_ptr(c + 1, 4 * kk + kq);
        }
        d4 acc[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
        // A[m][k] = Qm[k][m]  (Qs is [k][m]);  B[k][n] = X[k][n]
#pragma unroll
        for (int kk = 0; kk < JP / 4; ++kk) {
            const double a0 = ap0[kk * 4 * QS], a1 = ap1[kk * 4 * QS];
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, xb[kk], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, xb[kk], acc[1], 0, 0, 0);
        }
        const bool zero_null = c < cw; // deflated rows are zeroed in W only
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i * 16 + (lane >> 4) + 4 * r;
                const double val = (zero_null && zr[i][r]) ? 0.0 : acc[i][r];
                *chunk_ptr(c, row) = val;
            }
#pragma unroll
        for (int kk = 0; kk < JP / 4; ++kk) xb[kk] = xn[kk];
    }
}

// Kernel B of a round.  grid = pairs x U.
__global__ void __launch_bounds__(NT, 3)
jacobi_update_kernel(const JMat* __restrict__ mats, const JWork* __restrict__ work, int round, int U, JScratch sc, int buf,
                     int do_w, int do_j)
{
    __shared__ __attribute__((aligned(16))) double smem[JP * QS];
    __shared__ int zflag[JP];
    update_role(mats, work, round, blockIdx.x / U, blockIdx.x % U, U, sc, buf, do_w != 0, do_j != 0, smem, zflag);
}

// ================================================================================================
// Persistent sweep: ONE launch per sweep (all rounds of the round-robin schedule of every matrix).
//
// Workgroup (pair slot s of matrix m, column part g) stays on its CU for the whole sweep and walks the rounds
// r = 0 .. nb_m - 2 itself.  What used to be a kernel boundary between two rounds is a DATAFLOW hand-off: the rows of
// block P (column share g) updated in round r by the workgroup that held P then are picked up in round r + 1 by the
// workgroup whose slot the schedule moves P to -- same part g, so every (block, part) piece has exactly one owner per
// round and ownership travels with a monotonic counter  ready[block][part] = rounds completed  (Guideline 16: the piece
// is stored write-through (sc1), every storing wave drains, barrier, ONE lane publishes the counter; the next owner polls
// it with ONE lane, barrier, then reads the piece with sc1 loads).  Consequences:
//   * no launch ramp / drain / descriptor fetch per round (8-10 us of a 44 us round with a launch of its own);
//   * matrices are DECOUPLED: a small block never waits for a large one and vice versa -- the lockstep of a
//     launch per round makes every round as slow as its slowest pair and keeps the small blocks' pairs (most of the
//     pairs of a theta list) in the large blocks' rounds;
//   * parts per pair are chosen per matrix (long chains get the CUs): G_m in RPair.pad[0].
//
// A round of a workgroup.  The G workgroups of a block pair own disjoint COLUMN shares of the pair's 32 rows (whole
// 64-column chunks of W, and of J) for the whole launch:
//   0. wait for the two row blocks (above); every global load of the round is issued as early as its place in the load
//      queue allows: the own W share in Gram layout and -- for shares of up to SW_PRE chunks -- the own W / J share in
//      update layout, which waits in registers behind the eigensolve
//   1. partial Gram over the own W share (MFMA, operands straight from memory)
//   2. G > 1: the parts EXCHANGE their 32x32 partials and every part sums the G partials in the same fixed order --
//      bit-identical Gram matrices in all of them.  Two forms (template parameter GRAN).  Ticket form: every part publishes
//      its partial with 16-byte write-through stores, every storing wave drains, ONE lane adds an arrival ticket for the
//      workgroup and polls it (bounded) until all G have arrived, workgroup barrier, then every part reads the G partials
//      with 16-byte sc1 loads, all in flight at once.  Granule form: the data is the flag (see step 2 in the kernel).
//      In both the partials are DOUBLE BUFFERED by round parity, and the ticket is monotonic (target G (r + 1)): a part
//      can be at most one exchange ahead of its partners -- it cannot store round r + 2 before its own wait of round r + 1
//      has seen every partner's partial of r + 1, which a partner publishes only after it has read those of round r -- so
//      nobody still reads the buffer a store overwrites, and nothing is reset between rounds.
//   3. deflation test, convergence measure, two-sided Jacobi eigensolve of the 32x32 Gram, REDUNDANTLY in every part
//      (the chip is idle otherwise; no second exchange, no publish of Qm).  Template parameter RP: test and measure share
//      ONE interval between two barriers and work from the registers that hold the sums, a cross candidate's Gram is written
//      in interleaved positions at once, the rows are ranked on all four waves, and step 4 reads Qm from V through perm
//   4. X <- Qm^T X on the own column share of W and J, in place, then the hand-off of the two row blocks
// No workgroup reads or writes a column another workgroup of the launch touches, so within a round rows need no hand-off;
// the only data that cross between the parts of a pair are the 8 KB partials.
//
// Eigensolver: the Gram matrix and the accumulated rotations live in LDS in POSITION space -- thread (pr, pc) always owns
// the 2x2 block at block position (pr, pc), the matrix is physically permuted by the writes of every step (Brent-Luk ring:
// position 0 fixed, the other 31 advance one place, ring_next), so a step is ONE LDS round trip (own block + the diagonal
// block that defines the thread's column rotation, derived branch-free by every thread; the row rotation comes from the lane
// that derived it as its column rotation), the 2x2 updates, eight scattered stores and one barrier: no schedule table.
// After 31 steps every index is back at its position.
//
// Every wait is bounded by the wall clock AND leaves as soon as any workgroup has raised the error word, so a lost partner
// turns into an error code within a second, never into a hang.  All workgroups must be resident: the host launches at most
// one per CU and the kernel's LDS request (more than half a CU's) admits no second one.
struct RPair {            // everything a workgroup needs to know about its pair: one 64-byte read
    double* W;
    double* J;            // may be null
    double tol, thr2;
    int32_t nvp, lenp, nb, nv;
    int32_t mat, slot;
    int32_t pad[2];
};
static_assert(sizeof(RPair) == 64, "RPair is read as one 64-byte descriptor");

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
union Q16 {               // one 16-byte memory word = two doubles
    u32x4 u;
    d2 d;
};

constexpr int VS = JP + 2;                                      // row stride of V in LDS (position space)
static_assert(sizeof(RPair) == kPlanPairBytes && sizeof(int2) == kPlanMapBytes && sizeof(PlanRange) == sizeof(int2), "descriptor image of jacobi_plan.h");

__device__ __forceinline__ int ring_next(int p)  // destination position of position p after one step
{
    if (p == 0) return 0;
    if (p == 1) return 2;
    if (p & 1) return p - 2;          // bottom row moves left
    return p == JP - 2 ? JP - 1 : p + 2; // top row moves right, its last place drops to the bottom row
}

// Branch-free form of jacobi_rot (same formulas): 1/sqrt by v_rsq_f64 + two coupled Goldschmidt steps that deliver
// sqrt and 1/(2 sqrt) together -- two dependent FMAs per step.  A thread derives its row AND its column rotation; without
// branches the two chains interleave (one wave per SIMD: every dependent f64 operation is ~16 exposed cycles).
// thr2: relative threshold -- a coupling with b^2 <= thr2 a d is left alone.  Without it two rows of EQUAL norm (a multiple
// singular value) are rotated by 45 degrees on a coupling of pure rounding noise, which drags the not-yet-annihilated couplings
// of one into the other at FIRST order: convergence in the presence of clusters turns linear, and the prediction of the last
// sweep (jacobi_orthogonalise) left 3e-10 ... 8e-10 of non-orthogonality behind on blocks with eight-fold values
// (scripts/svd_fuzz.py).  The callers pass (tol / 2)^2: such a pair counts as converged anyway.
__device__ __forceinline__ void jacobi_rot_bf(double a, double d, double b, double& c, double& s, double thr2 = 0.0)
{
    const double delta = d - a;
    const double b2 = b + b;
    double h2 = fma(b2, b2, delta * delta);
    const bool ok = (fabs(b) > 1e-300) & (h2 > 1e-300) & (b * b > thr2 * a * d);
    h2 = ok ? h2 : 1.0;
    double r = __builtin_amdgcn_rsq(h2);
    double g = h2 * r, h = 0.5 * r;
    double e = fma(-g, h, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
    e = fma(-g, h, 0.5);
    h = fma(h, e, h);                             // 1 / (2 hyp)
    const double c2 = fma(fabs(delta), h, 0.5);   // cos^2 theta in [1/2, 1]
    double r2 = __builtin_amdgcn_rsq(c2);
    double gc = c2 * r2, hc = 0.5 * r2;
    double ec = fma(-gc, hc, 0.5);
    gc = fma(gc, ec, gc);
    hc = fma(hc, ec, hc);
    ec = fma(-gc, hc, 0.5);
    gc = fma(gc, ec, gc);                         // cos theta
    hc = fma(hc, ec, hc);                         // 1 / (2 cos theta)
    const double sabs = (fabs(b) * h) * (4.0 * hc); // |b| / (hyp cos theta)
    const bool pos = (delta >= 0.0) == (b >= 0.0);
    c = ok ? gc : 1.0;
    s = ok ? (pos ? sabs : -sabs) : 0.0;
}


// Structure-preserving pivot solve for the interleaved real embedding of COMPLEX rows: the
// 32 x 32 Gram matrix of a pair of 16-row blocks -- 8 + 8 complex rows, real row 2a (+1) = real (imaginary) embedding row of
// complex row a -- is M(G_c) of a 16 x 16 Hermitian G_c.  One wave diagonalises G_c by cyclic complex Jacobi rotations in
// LDS and leaves M(Q_c) and M(Lambda): the real update that follows then IS the complex one, rows stay structured and every
// singular value appears once per complex row.  A rotation for the Hermitian 2 x 2 [[a, g], [conj g, d]] is the real Jacobi
// rotation of [[a, |g|], [|g|, d]] behind the phase g / |g|:  U = [[c, s], [-s conj(phi), c conj(phi)]].
constexpr int CJ = JP / 2;  // complex rows per pair problem
constexpr int CS = CJ + 1;  // row stride of the complex work arrays
__device__ __forceinline__ void hermitian_pivot_solve(const double* Gs, double* work, double* rot, double* Vout, double* Gdiag, int sweeps,
                                                      int lane, double thr2 = 0.0, bool cross = false)
{   // work: 4 * CJ * CS doubles;  rot: 2 * CJ doubles (CJ/2 rotations x c, s, phi_re, phi_im)
    // cross: only the CJ/2 rotation sets that pair a complex row of block P (0 .. CJ/2 - 1) with one of block Q (SScratch::cross_every)
    auto pair_of = [cross](int r, int k, int& p, int& q) {
        if (cross) {
            p = k;
            q = CJ / 2 + ((k + r) & (CJ / 2 - 1));
        } else
            circle_pair(CJ, r, k, p, q);
    };
    const int n_steps = cross ? CJ / 2 : CJ - 1;
    double* Hr = work;                 // [CJ][CS] each
    double* Hi = Hr + CJ * CS;
    double* Ur = Hi + CJ * CS;
    double* Ui = Ur + CJ * CS;
    for (int e = lane; e < CJ * CJ; e += 64) {
        const int a = e / CJ, b = e % CJ;
        // M(G_c)[2a][2b] = Re, M(G_c)[2a+1][2b] = Im; the two copies of every entry differ by rounding: average them
        Hr[a * CS + b] = 0.5 * (Gs[(2 * a) * GS + 2 * b] + Gs[(2 * a + 1) * GS + 2 * b + 1]);
        Hi[a * CS + b] = a == b ? 0.0 : 0.5 * (Gs[(2 * a + 1) * GS + 2 * b] - Gs[(2 * a) * GS + 2 * b + 1]);
        Ur[a * CS + b] = a == b ? 1.0 : 0.0;
        Ui[a * CS + b] = 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int sw = 0; sw < sweeps; ++sw)
        for (int r = 0; r < n_steps; ++r) {
            if (lane < CJ / 2) {
                int p, q;
                pair_of(r, lane, p, q);
                const double gr = Hr[p * CS + q], gi = Hi[p * CS + q];
                const double ab = sqrt(gr * gr + gi * gi);
                double c = 1.0, sn = 0.0, pr = 1.0, pi = 0.0;
                if (ab > 1e-300) {
                    jacobi_rot_bf(Hr[p * CS + p], Hr[q * CS + q], ab, c, sn, thr2);
                    pr = gr / ab;
                    pi = gi / ab;
                }
                rot[lane * 4 + 0] = c;
                rot[lane * 4 + 1] = sn;
                rot[lane * 4 + 2] = pr;
                rot[lane * 4 + 3] = pi;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // rows:  row_p <- c row_p - s phi row_q,   row_q <- s row_p + c phi row_q        (H <- U^H H)
            for (int e = lane; e < (CJ / 2) * CJ; e += 64) {
                const int k = e / CJ, col = e % CJ;
                int p, q;
                pair_of(r, k, p, q);
                const double c = rot[k * 4], sn = rot[k * 4 + 1], fr = rot[k * 4 + 2], fi = rot[k * 4 + 3];
                const double pr_ = Hr[p * CS + col], pi_ = Hi[p * CS + col], qr_ = Hr[q * CS + col], qi_ = Hi[q * CS + col];
                const double tr = fr * qr_ - fi * qi_, ti = fr * qi_ + fi * qr_; // phi * row_q
                Hr[p * CS + col] = c * pr_ - sn * tr;
                Hi[p * CS + col] = c * pi_ - sn * ti;
                Hr[q * CS + col] = sn * pr_ + c * tr;
                Hi[q * CS + col] = sn * pi_ + c * ti;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // columns of H and of U:  col_p <- c col_p - s conj(phi) col_q,   col_q <- s col_p + c conj(phi) col_q   (. <- . U)
            for (int e = lane; e < (CJ / 2) * CJ * 2; e += 64) {
                const int which = e / ((CJ / 2) * CJ), f = e % ((CJ / 2) * CJ);
                const int k = f / CJ, row = f % CJ;
                int p, q;
                pair_of(r, k, p, q);
                double* Xr = which ? Ur : Hr;
                double* Xi = which ? Ui : Hi;
                const double c = rot[k * 4], sn = rot[k * 4 + 1], fr = rot[k * 4 + 2], fi = -rot[k * 4 + 3];
                const double pr_ = Xr[row * CS + p], pi_ = Xi[row * CS + p], qr_ = Xr[row * CS + q], qi_ = Xi[row * CS + q];
                const double tr = fr * qr_ - fi * qi_, ti = fr * qi_ + fi * qr_; // conj(phi) * col_q
                Xr[row * CS + p] = c * pr_ - sn * tr;
                Xi[row * CS + p] = c * pi_ - sn * ti;
                Xr[row * CS + q] = sn * pr_ + c * tr;
                Xi[row * CS + q] = sn * pi_ + c * ti;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    // expand: Vout[k][j] (row stride VS) = M(U)[k][j],  Gdiag[i][i] (row stride GS) = lambda_{i / 2}
    for (int e = lane; e < CJ * CJ; e += 64) {
        const int a = e / CJ, b = e % CJ;
        const double x = Ur[a * CS + b], y = Ui[a * CS + b];
        Vout[(2 * a) * VS + 2 * b] = x;
        Vout[(2 * a) * VS + 2 * b + 1] = -y;
        Vout[(2 * a + 1) * VS + 2 * b] = y;
        Vout[(2 * a + 1) * VS + 2 * b + 1] = x;
    }
    if (lane < CJ) {
        const double lam = Hr[lane * CS + lane];
        Gdiag[(2 * lane) * GS + 2 * lane] = lam;
        Gdiag[(2 * lane + 1) * GS + 2 * lane + 1] = lam;
    }
}

struct SScratch {
    double* gpart;            // [pair][2][G_max][JP*JP]
    unsigned int* ticket;     // [pair]                 arrivals of the Gram exchange (zeroed per sweep)
    unsigned int* ready;      // [matrix flag base + block * G + part]   rounds completed (zeroed per sweep)
    unsigned int* err;        // [1]
    const int2* wgmap;        // [entry] -> (pair, part)
    const int2* wgent;        // [workgroup] -> [begin, end) of its entries in wgmap (null: workgroup b owns entry b).  More than
                              // one entry per workgroup: lists with more pairs than the chip has CUs -- a workgroup then runs its
                              // entries one after the other in every round (short matrices share, long chains stay alone)
    unsigned long long* stamps;
    int stamp_round;
    // all sweeps in ONE launch (n_sweeps > 1): the convergence test runs on the device.  offmax_bits is then [sweep][matrix];
    // arrive[matrix] counts the (pair, part) entries of a matrix that have finished a sweep (monotonic), nsw[matrix] is the
    // number of sweeps the matrix took (0: not converged within n_sweeps)
    int n_sweeps, n_mats;
    unsigned int* arrive;
    int* nsw;
    // Deferred J update: a workgroup applies a round's rotation to its W share at once (the next owners wait for that), and to
    // its J share only while it waits for the partial Grams of the NEXT round -- nobody reads J before the end, so that half of
    // the update fills what was idle time.  readyJ[block][part]: rounds whose J update (or skip) is complete, as `ready` for W.
    unsigned int* readyJ;
    int defer_j;
    // Granule form of the Gram exchange (template parameter GRAN): [part of the launch][round parity] regions of SW_GRAN_U64
    // tagged words each, zeroed with the counters before every launch.  A matrix's regions start at unit
    // (RPair.pad[1] - gran_np), its pair `slot` at 2 * slot * G behind that: [parity][part].
    unsigned long long* gran;
    int gran_np;
    // Cross-only pivot solves (real engine, one inner sweep): the 31 rotation sets of a pivot solve are 16 sets of pairs (row of
    // block P, row of block Q) and 15 sets of pairs inside a block.  A sweep needs every pair of rows ONCE; the pairs inside a
    // block are met again in every round the block takes part in.  With cross_every = k > 0 only the rounds with round % k == 0
    // run all 31 sets, the others the 16 cross sets (positions interleaved P0 Q0 P1 Q1 ..., the Q side moves one place per step).
    int cross_every, cross_min_nb;
};
constexpr int SW_MAX_ENT = 64; // entries per workgroup the one-launch form keeps a done flag for

constexpr int SW_UN = 8;                                        // 8-column Gram chunks in flight per wave and buffer
constexpr int SW_PRE = 6;                                       // update chunks held in registers across the eigensolve
// One partial Gram as granules: every double is two 8-byte words {tag, low half} {tag, high half} (tag in the upper 32 bits),
// each written by ONE aligned 8-byte store and read by one 8-byte load.
constexpr int SW_GRAN_U64 = 2 * JP * JP;
constexpr unsigned int SW_GRAN_BYTES = 8u * SW_GRAN_U64;
static_assert(SW_GRAN_BYTES == kPlanGranBytes, "granule regions of jacobi_plan.h");
// [Gs | region shared by the wave slices of the partial Gram (Xc) and the eigensolver's G2 / Va / Vb | Qm of this round and of the
//  previous one (the deferred J update still reads it while the next Gram runs) | reduction scratch]
constexpr int SWEEP_XREG = (4 * JP * GS > JP * GS + 2 * JP * VS) ? 4 * JP * GS : JP * GS + 2 * JP * VS;
constexpr int SWEEP_LDS_DOUBLES = JP * GS + SWEEP_XREG + 2 * JP * QS + 8;
// ONE workgroup per CU (the LDS request is padded past half a CU's 160 KB).  Two per CU were measured and dropped: with the
// 256-register budget that needs (SW_UN = 2, SW_PRE = 2: no spills) and twice the parts per pair, a round of the largest
// block of the chi=4096 list took 44.5 us instead of 46 (eigensolve 19.5 instead of 16.7 us with a second wave on every
// SIMD, exchange among 8 parts 11 instead of 6.5 us) and the batched SVD 52.3 instead of 49.9 ms.
constexpr size_t SWEEP_LDS_BYTES = 88 * 1024;
static_assert((size_t)SWEEP_LDS_DOUBLES * 8 + 1024 <= SWEEP_LDS_BYTES, "LDS request of the sweep kernel");
constexpr int SWEEP_WG_PER_CU = 1;

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
union Q8 {
    u32x2 u;
    double d;
};

template <int SLEEP = 1>
__device__ __forceinline__ bool spin_until(const unsigned int* word, unsigned int target, unsigned int* err)
{
    const unsigned long long t0 = wall_clock64(); // 100 MHz
    unsigned int it = 0;
    while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(SLEEP);
        if ((++it & 63u) == 0u) {
            if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return false;
            if (wall_clock64() - t0 > 100000000ull) { // one second
                __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return false;
            }
        }
    }
    return true;
}

// Both words of a hand-off at once: the two loads are in flight together, ONE round trip when both counters are already
// there (the serial form pays two dependent ones).  Same bound and error word; false when either word fails.
template <int SLEEP = 1>
__device__ __forceinline__ bool spin_until2(const unsigned int* word0, const unsigned int* word1, unsigned int target, unsigned int* err)
{
    const unsigned long long t0 = wall_clock64(); // 100 MHz
    unsigned int it = 0;
    for (;;) {
        const unsigned int v0 = __hip_atomic_load(word0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned int v1 = __hip_atomic_load(word1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((v0 >= target) & (v1 >= target)) return true;
        __builtin_amdgcn_s_sleep(SLEEP);
        if ((++it & 63u) == 0u) {
            if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return false;
            if (wall_clock64() - t0 > 100000000ull) { // one second
                __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return false;
            }
        }
    }
}
// RORD: the round's issue order of this file (false: the order it had before, kept for A/B -- CYB_JACOBI_ROUND_ORDER=0)
template <bool RORD>
__device__ __forceinline__ bool spin_pair(const unsigned int* word0, const unsigned int* word1, unsigned int target, unsigned int* err)
{
    if constexpr (RORD) return spin_until2(word0, word1, target, err);
    else return spin_until(word0, target, err) && spin_until(word1, target, err);
}

// J rows of the pair (P, Q), column chunks [j_begin, j_begin + nJ) of 64:  X <- Qm^T X  (Qm in LDS as [k][m], stride QS)
__device__ __forceinline__ void sweep_update_j(const __amdgpu_buffer_rsrc_t rsJ, const double* Qm, int P, int Q, int nvp, int j_begin,
                                               int nJ, int wave, int lane)
{
    const int un = lane & 15, ukq = lane >> 4;
    const double* ap0 = Qm + (lane >> 4) * QS + (lane & 15);
    const double* ap1 = ap0 + 16;
    double a0[JP / 4], a1[JP / 4];
#pragma unroll
    for (int kk = 0; kk < JP / 4; ++kk) {
        a0[kk] = ap0[kk * 4 * QS];
        a1[kk] = ap1[kk * 4 * QS];
    }
    auto off_of = [&](int c, int k) { return (unsigned int)(((int64_t)xrow(k, P, Q) * nvp + (j_begin + c) * 64 + wave * 16 + un) * 8); };
    auto load = [&](double (&x)[JP / 4], int c) {
#pragma unroll
        for (int kk = 0; kk < JP / 4; ++kk) {
            Q8 q;
            q.u = __builtin_amdgcn_raw_buffer_load_b64(rsJ, off_of(c, 4 * kk + ukq), 0, 16);
            x[kk] = q.d;
        }
    };
    double xb[JP / 4], xn[JP / 4];
    if (nJ > 0) load(xb, 0);
    for (int c = 0; c < nJ; ++c) {
        if (c + 1 < nJ) load(xn, c + 1);
        d4 acc[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
        for (int kk = 0; kk < JP / 4; ++kk) {
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[kk], xb[kk], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[kk], xb[kk], acc[1], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                Q8 v;
                v.d = acc[i][q];
                __builtin_amdgcn_raw_buffer_store_b64(v.u, rsJ, off_of(c, i * 16 + (lane >> 4) + 4 * q), 0, 16);
            }
#pragma unroll
        for (int kk = 0; kk < JP / 4; ++kk) xb[kk] = xn[kk];
    }
}

// GRAN: the partial Grams travel as tagged granules (step 2; false: stores, drain, ticket and poll as before, kept for
// A/B -- CYB_JACOBI_EXCHANGE=0)
// RP: the LDS passes around the pivot solve in their folded form (steps 3a-3c and the head of step 4; false: the passes and
// barriers as before, kept for A/B -- CYB_JACOBI_ROUND_PASSES=0).  Only the default order and exchange have the folded form.
template <bool CPLX, bool RORD, bool GRAN, bool RP>
__global__ void __launch_bounds__(NT, 1)
jacobi_sweep_kernel(const RPair* __restrict__ pairs, int max_inner, unsigned long long* __restrict__ offmax_bits, SScratch sc)
{
    static_assert(!RP || (RORD && GRAN), "the folded passes exist for the default round order and exchange only");
    extern __shared__ __attribute__((aligned(16))) double rsm[];
    // LDS carve-up for two to three workgroups per CU: the wave slices of the partial Gram (Xc) are dead once the
    // exchange has produced Gs, so they share their space with the eigensolver's second Gram buffer, V and Qs
    double* Gs = rsm;
    double* G2 = Gs + JP * GS;
    double* Va = G2 + JP * GS;
    double* Vb = Va + JP * VS;
    double* Xc = G2;                                        // (SWEEP_XREG doubles: the larger of the two uses)
    double* Qs0 = G2 + SWEEP_XREG;                          // Qm of even rounds ...
    double* Qs1 = Qs0 + JP * QS;                            // ... and of odd ones (counted per matrix: `ground`)
    double* red = Qs1 + JP * QS;
    int* ibase = reinterpret_cast<int*>(red + 8);
    int* perm = ibase;
    int* zrow = ibase + JP;
    int* zout = ibase + 2 * JP;
    int* flags = ibase + 3 * JP; // [0] any null  [1] wait ok  [2] every entry of this workgroup has converged  [3] a granule sweep gave up
    int* edone = flags + 4;      // [SW_MAX_ENT] one-launch form: entry has converged

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int2 went = sc.wgent ? sc.wgent[blockIdx.x] : make_int2((int)blockIdx.x, (int)blockIdx.x + 1);
    int max_rounds = 0;
    for (int e = went.x; e < went.y; ++e) max_rounds = max(max_rounds, pairs[sc.wgmap[e].x].nb - 1);
    const int n_sw = sc.n_sweeps;
    // deferred J update (workgroups with ONE entry: pair slot and part are then the same in every round)
    const bool one_entry = went.y - went.x == 1;
    int pendP = -1, pendQ = -1, pend_ground = 0; // J update of an earlier round still to be applied (pendP < 0: none)
    if (n_sw > 1) {
        if (tid < SW_MAX_ENT) edone[tid] = 0;
        __syncthreads();
    }
    for (int sw = 0; sw < n_sw; ++sw) {
    for (int round = 0; round < max_rounds; ++round)
    for (int ent = went.x; ent < went.y; ++ent) {
    const int2 wm = sc.wgmap[ent];
    const int pi = wm.x, part = wm.y;
    const RPair mt = pairs[pi];
    if (round >= mt.nb - 1) continue; // (workgroup-uniform)
    if (n_sw > 1 && edone[ent - went.x]) continue;
    const int ground = sw * (mt.nb - 1) + round; // rounds this matrix has been through (counters and buffers never reset)
    const int G = mt.pad[0];
    unsigned int* ready = sc.ready + mt.pad[1];
    unsigned int* readyJ = sc.readyJ + mt.pad[1];
    unsigned int* ticket = sc.ticket + pi;
    double* Qs = (ground & 1) ? Qs1 : Qs0;
    const unsigned int pbytes = JP * JP * 8;
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(mt.W, 0, (int)((size_t)mt.nvp * mt.lenp * 8), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsJ =
        __builtin_amdgcn_make_buffer_rsrc(mt.J ? mt.J : mt.W, 0, mt.J ? (int)((size_t)mt.nvp * mt.nvp * 8) : 0, 0x00020000);
    // column shares in whole 64-column chunks (fixed for the sweep)
    const int cw = mt.lenp / 64, cj = mt.J ? mt.nvp / 64 : 0;
    const int w_begin = (int)((int64_t)part * cw / G), w_end = (int)((int64_t)(part + 1) * cw / G);
    const int j_begin = (int)((int64_t)part * cj / G), j_end = (int)((int64_t)(part + 1) * cj / G);
    const int nW = w_end - w_begin, nJ = j_end - j_begin;
    // this round's J half is deferred into the exchange wait of the next round (needs an exchange: G > 1)
    const bool defer = sc.defer_j && one_entry && G > 1 && nJ > 0 && round < mt.nb - 2; // (the last round of a sweep updates J at once)
    const int ct = defer ? nW : nW + nJ;
    const int pre_limit = (sc.defer_j && G > 1) ? min(ct, nW) : ct; // chunks that may be prefetched before the eigensolve
    const int un = lane & 15, ukq = lane >> 4;
#define SWEEP_STAMP(k)                                                                                            \
    do {                                                                                                          \
        if (sc.stamps && tid == 0 && round == sc.stamp_round) sc.stamps[(size_t)blockIdx.x * 8 + (k)] = wall_clock64(); \
    } while (0)

    {
        int P, Q;
        circle_pair(mt.nb, round, mt.slot, P, Q);
        if (P > Q) {
            const int t = P;
            P = Q;
            Q = t;
        }
        SWEEP_STAMP(0);
        // ---- 0. take over the two row blocks: their previous owners have finished round - 1
        __syncthreads(); // (also: nobody still reads the LDS of the previous round)
        if (ground > 0) {
            if (tid == 0) {
                flags[1] = spin_pair<RORD>(ready + (size_t)P * G + part, ready + (size_t)Q * G + part, (unsigned int)ground, sc.err) ? 1 : 0;
            }
            __syncthreads();
            if (!flags[1]) return;
        }
        SWEEP_STAMP(1);
        if constexpr (GRAN) {
            if (tid == 0) flags[3] = 0; // (read behind the barrier that ends step 2; two barriers lie between)
        }
        if constexpr (RP) {
            if (tid == 0) flags[0] = 0; // (raised in step 3a behind the barrier that ends step 2, last read before the round's end)
        }
        // Everything that decides a cross-only solve except the null rows is known here (the same in every part)
        // (cross_every < 0: adaptive -- at least four full rounds per sweep of a matrix, whatever its block count)
        const int cross_k = sc.cross_every > 0 ? sc.cross_every : max(4, (mt.nb + 2) / 4);
        const bool cross_terms = sc.cross_every != 0 && mt.nb >= sc.cross_min_nb && (round % cross_k) != 0;
        auto cpos = [](int i) { return i < JB ? 2 * i : 2 * (i - JB) + 1; };     // index -> interleaved position
        auto cidx = [](int p) { return (p & 1) ? JB + (p >> 1) : (p >> 1); };    // interleaved position -> index
        // RP: a cross candidate's Gram is WRITTEN in interleaved positions (there is no natural copy; the rare round with a null
        // row writes it again from the registers)
        const bool ilv = RP && !CPLX && cross_terms;
        double gv[4] = {0.0, 0.0, 0.0, 0.0};                                     // RP: the four sums of this thread (row gi, columns gj ..)
        // byte offset of element (row k of the pair, own chunk c, column un of this wave's 16) and its descriptor
        auto chunk_off = [&](int c, int k, bool& in_w) -> unsigned int {
            in_w = c < nW;
            const int ld = in_w ? mt.lenp : mt.nvp;
            const int cc = in_w ? w_begin + c : j_begin + (c - nW);
            return (unsigned int)(((int64_t)xrow(k, P, Q) * ld + cc * 64 + wave * 16 + un) * 8);
        };
        auto chunk_load = [&](int c, int k) -> double {
            bool in_w;
            const unsigned int off = chunk_off(c, k, in_w);
            Q8 q;
            q.u = in_w ? __builtin_amdgcn_raw_buffer_load_b64(rsW, off, 0, 16) : __builtin_amdgcn_raw_buffer_load_b64(rsJ, off, 0, 16);
            return q.d;
        };
        // ---- 1. partial Gram over the own W share
        double xpre[SW_PRE][JP / 4];
        // The update's operands: nothing reads them before the pivot solve has ended.  Loads return in order and a wave stalls
        // once the queue is full, so WHERE they are issued decides what waits behind them (see step 2).
        auto issue_xpre = [&]() {
#pragma unroll
            for (int c = 0; c < SW_PRE; ++c) {
                if (c < pre_limit) { // (J chunks of a matrix whose J updates may be deferred are loaded after the wait for them)
#pragma unroll
                    for (int kk = 0; kk < JP / 4; ++kk) xpre[c][kk] = chunk_load(c, 4 * kk + ukq);
                }
            }
        };
        {
            const int ld = mt.lenp;
            d4 acc00 = d4{0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc11 = acc00;
            const int r = lane & 15, g2 = 2 * (lane >> 4);
            const unsigned int o0 = (unsigned int)(((int64_t)xrow(r, P, Q) * ld + g2) * 8);
            const unsigned int o1 = (unsigned int)(((int64_t)xrow(r + 16, P, Q) * ld + g2) * 8);
            const int c_begin = 8 * w_begin, c_end = 8 * w_end; // in 8-column chunks
            constexpr int UN = SW_UN;
            d2 x0[UN], x1[UN], n0[UN], n1[UN];
            auto load = [&](d2 (&a0)[UN], d2 (&a1)[UN], int c0) {
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    const int c = min(c0 + 4 * u, c_end - 1);
                    Q16 qa, qb;
                    qa.u = __builtin_amdgcn_raw_buffer_load_b128(rsW, o0 + (unsigned int)c * 64u, 0, 16);
                    qb.u = __builtin_amdgcn_raw_buffer_load_b128(rsW, o1 + (unsigned int)c * 64u, 0, 16);
                    a0[u] = qa.d;
                    a1[u] = qb.d;
                }
            };
            auto gram = [&](const d2 (&a0)[UN], const d2 (&a1)[UN], int c0) {
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    if (c0 + 4 * u < c_end) {
                        acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u].x, a0[u].x, acc00, 0, 0, 0);
                        acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u].x, a1[u].x, acc01, 0, 0, 0);
                        acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u].x, a1[u].x, acc11, 0, 0, 0);
                        acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u].y, a0[u].y, acc00, 0, 0, 0);
                        acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u].y, a1[u].y, acc01, 0, 0, 0);
                        acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u].y, a1[u].y, acc11, 0, 0, 0);
                    }
                }
            };
            if constexpr (RORD) {
                // Nothing but the Gram's own loads is queued here (loads return in order: an update operand between the
                // groups would sit ahead of the partial Gram the partners wait for).  The two buffers swap roles instead of
                // being copied, and the test for a next group is hoisted around the MFMA block, so that every path is
                // straight-line code and MFMA group u waits with a counted vmcnt for its own two loads only.
                int c0 = c_begin + wave;
                if (c0 < c_end) {
                    load(x0, x1, c0);
                    for (;;) {
                        if (c0 + 4 * UN < c_end) {
                            load(n0, n1, c0 + 4 * UN);
                            gram(x0, x1, c0);
                        } else {
                            gram(x0, x1, c0);
                            break;
                        }
                        c0 += 4 * UN;
                        if (c0 + 4 * UN < c_end) {
                            load(x0, x1, c0 + 4 * UN);
                            gram(n0, n1, c0);
                        } else {
                            gram(n0, n1, c0);
                            break;
                        }
                        c0 += 4 * UN;
                    }
                }
            } else {
            if (c_begin + wave < c_end) load(x0, x1, c_begin + wave);
            issue_xpre();
            for (int c0 = c_begin + wave; c0 < c_end; c0 += 4 * UN) {
                const bool more = c0 + 4 * UN < c_end;
                if (more) load(n0, n1, c0 + 4 * UN);
                gram(x0, x1, c0);
                if (more) {
#pragma unroll
                    for (int u = 0; u < UN; ++u) {
                        x0[u] = n0[u];
                        x1[u] = n1[u];
                    }
                }
            }
            }
            double* wpart = Xc + wave * (JP * GS);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rr = (lane >> 4) + 4 * q, cc = lane & 15;
                wpart[rr * GS + cc] = acc00[q];
                wpart[rr * GS + 16 + cc] = acc01[q];
                wpart[(16 + cc) * GS + rr] = acc01[q];
                wpart[(16 + rr) * GS + 16 + cc] = acc11[q];
            }
        }
        __syncthreads();
        SWEEP_STAMP(2);
        // The Gram loop leaves loads nobody consumes (the clamped tail of its last group).  They have landed by now, but the
        // compiler's wait counting cannot know (it does not see the drains written as inline assembly), and drains the queue
        // -- the prefetch below included -- at the first reuse of one of their registers, after the exchange or inside the
        // pivot solve.  Hence a wait it can see: the builtin.
        if constexpr (RORD) __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
        {
            const int gi = tid >> 3, gj = 4 * (tid & 7);
            d2 lo = d2{0.0, 0.0}, hi = d2{0.0, 0.0};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const double* src = Xc + w * (JP * GS) + gi * GS + gj;
                lo.x += src[0];
                lo.y += src[1];
                hi.x += src[2];
                hi.y += src[3];
            }
            // ---- 2. exchange of the partials among the G parts (double buffered by round parity)
            const __amdgpu_buffer_rsrc_t rs_all = __builtin_amdgcn_make_buffer_rsrc(
                sc.gpart + ((size_t)pi * 2 + (size_t)(ground & 1)) * RGMAX * (JP * JP), 0, (int)(pbytes * G), 0x00020000);
            // Granule form: the data is the flag.  Every 32-bit half of a partial travels in an 8-byte word {tag, half}, written
            // by ONE aligned 8-byte agent-scope store (write-through), tag = ground + 1: counted within the launch, never 0
            // (the regions are zeroed before every launch), different in every round this pair runs in the launch.  No drain,
            // no barrier, no ticket: a consumer re-reads the words until every tag is this round's and then holds the data.
            // The regions are double buffered by round parity like the slabs of the ticket form, by the same argument: a
            // part stores round g + 2 only after its own sweep of round g + 1 has seen every partner's words of g + 1, and a
            // partner stores those only after its sweep of round g has ended -- nobody still reads what g + 2 overwrites, and
            // a reader of round g can meet the tags g - 1 (or 0) and g + 1 only.
            const unsigned int gtag = (unsigned int)(ground + 1);
            GLOBAL_AS unsigned long long* gran_pair =
                (GLOBAL_AS unsigned long long*)sc.gran +
                ((size_t)(mt.pad[1] - sc.gran_np) + (size_t)(2 * mt.slot + (ground & 1)) * (size_t)G) * SW_GRAN_U64;
            if constexpr (GRAN) {
                if (G > 1) {
                    // word j of lane l of wave w sits at [w][j][l]: the 64 lanes of a store fill 512 contiguous bytes
                    // (thread-major, 64 partial lines per store: exchange 8.3 us)
                    GLOBAL_AS unsigned long long* mine = gran_pair + (size_t)part * SW_GRAN_U64 + (size_t)(wave * 512 + lane);
                    const double v[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        __hip_atomic_store(mine + 128 * k, ((unsigned long long)gtag << 32) | (unsigned int)__double2loint(v[k]), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(mine + 128 * k + 64, ((unsigned long long)gtag << 32) | (unsigned int)__double2hiint(v[k]), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            } else if (G > 1) {
                Q16 a, b;
                a.d = lo;
                b.d = hi;
                const unsigned int off = (unsigned int)part * pbytes + (unsigned int)tid * 32u;
                __builtin_amdgcn_raw_buffer_store_b128(a.u, rs_all, off, 0, 16);
                __builtin_amdgcn_raw_buffer_store_b128(b.u, rs_all, off + 16u, 0, 16);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // The update's operands go out HERE: behind the ticket (granule form: behind the granule stores), so that nothing the
            // partners wait for queues behind them, and in front of the poll (the first granule sweep), so that their issue (48
            // loads per lane fill the queue: the wave stalls) falls into the wait for the partners' tickets (words).  Issued behind the loads of the partners' partials instead, the sum of the
            // partials waited for that issue (exchange 5.9 -> 8.5 us).  They land during the poll; the barriers of the pivot
            // solve carry no vmcnt wait.  ONE site for every G (without an exchange it follows the Gram loop): two sites
            // meet in register copies, i.e. in a wait for the loads just issued.
            if constexpr (RORD) issue_xpre();
            if (G > 1) {
                if (pendP >= 0) {
                    // ---- the J half of the previous round's update, while the partners' partial Grams are on their way
                    if (tid == 0) {
                        flags[1] = spin_pair<RORD>(readyJ + (size_t)pendP * G + part, readyJ + (size_t)pendQ * G + part, (unsigned int)pend_ground, sc.err) ? 1 : 0;
                    }
                    __syncthreads();
                    if (!flags[1]) return;
                    sweep_update_j(rsJ, (pend_ground & 1) ? Qs1 : Qs0, pendP, pendQ, mt.nvp, j_begin, nJ, wave, lane);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    if (tid == 0) {
                        __hip_atomic_store(readyJ + (size_t)pendP * G + part, (unsigned int)(pend_ground + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(readyJ + (size_t)pendQ * G + part, (unsigned int)(pend_ground + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    pendP = -1;
                }
                const d2 own_lo = lo, own_hi = hi;
                lo = d2{0.0, 0.0};
                hi = d2{0.0, 0.0};
                if constexpr (GRAN) {
                    // Every thread sweeps the eight words of its own four elements in the partners' parts (its own partial comes
                    // from its registers, at its place in the order of the sum), four parts in flight as in the ticket form, with 8-byte
                    // write-through-aware loads to registers at the offsets it stores to (512 contiguous bytes per wave and
                    // load), and repeats a group of parts until the wave has seen this round's tag on every word.  Bounded
                    // like spin_until: one second, the same error word; a wave that gives up raises flags[3] and the workgroup
                    // leaves behind the barrier that ends this step.
                    const __amdgpu_buffer_rsrc_t rs_gran = __builtin_amdgcn_make_buffer_rsrc((unsigned long long*)gran_pair, 0, (int)(SW_GRAN_BYTES * G), 0x00020000);
                    const unsigned long long t0 = wall_clock64(); // 100 MHz
                    unsigned int it = 0, passes = 0;
                    bool good = true;
                    for (int g0 = 0; g0 < G && good; g0 += 4) {
                        u32x2 w[4][8];
                        for (;;) {
                            asm volatile("" ::: "memory"); // (every pass loads anew)
                            unsigned int bad = 0u; // (branch-free: nonzero when some tag is not this round's)
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                if (g0 + g < G && g0 + g != part) {
#pragma unroll
                                    for (int j = 0; j < 8; ++j)
                                        // (addresses that do not depend on the part: it goes into the scalar offset -- an address
                                        //  register written between two loads costs a wait for the loads in flight)
                                        w[g][j] = __builtin_amdgcn_raw_buffer_load_b64(rs_gran, (unsigned int)(wave * 4096 + lane * 8) + 512u * j, (g0 + g) * (int)SW_GRAN_BYTES, 16);
                                }
                            }
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                if (g0 + g < G && g0 + g != part) {
#pragma unroll
                                    for (int j = 0; j < 8; ++j) bad |= w[g][j][1] ^ gtag;
                                }
                            }
                            ++passes;
                            if (__all(bad == 0u)) break;
                            __builtin_amdgcn_s_sleep(1);
                            if ((++it & 63u) == 0u) {
                                if (__hip_atomic_load(sc.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) good = false;
                                else if (wall_clock64() - t0 > 100000000ull) { // one second
                                    __hip_atomic_store(sc.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    good = false;
                                }
                                if (!good) break;
                            }
                        }
                        if (!good) break;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            if (g0 + g == part) { // (the own partial never left its registers; it takes its place in the order)
                                lo += own_lo;
                                hi += own_hi;
                            } else if (g0 + g < G) {
                                lo.x += __hiloint2double((int)w[g][1][0], (int)w[g][0][0]);
                                lo.y += __hiloint2double((int)w[g][3][0], (int)w[g][2][0]);
                                hi.x += __hiloint2double((int)w[g][5][0], (int)w[g][4][0]);
                                hi.y += __hiloint2double((int)w[g][7][0], (int)w[g][6][0]);
                            }
                        }
                    }
                    if (!good && lane == 0) flags[3] = 1;
                    if (sc.stamps && tid == 0 && round == sc.stamp_round) sc.stamps[(size_t)blockIdx.x * 8 + 7] = passes; // (diagnostic: passes of wave 0)
                } else {
                if (tid == 0) flags[1] = spin_until(ticket, (unsigned int)G * (unsigned int)(ground + 1), sc.err) ? 1 : 0;
                __syncthreads();
                if (!flags[1]) return;
                for (int g0 = 0; g0 < G; g0 += 4) { // four parts' loads in flight at a time; the same order in every part
                    Q16 pa[4], pb[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        if (g0 + g < G) {
                            pa[g].u = __builtin_amdgcn_raw_buffer_load_b128(rs_all, (unsigned int)(g0 + g) * pbytes + (unsigned int)tid * 32u, 0, 16);
                            pb[g].u = __builtin_amdgcn_raw_buffer_load_b128(rs_all, (unsigned int)(g0 + g) * pbytes + (unsigned int)tid * 32u + 16u, 0, 16);
                        }
                    }
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        if (g0 + g < G) {
                            lo += pa[g].d;
                            hi += pb[g].d;
                        }
                    }
                }
                } // (ticket form)
            }
            if constexpr (RP) {
                gv[0] = lo.x;
                gv[1] = lo.y;
                gv[2] = hi.x;
                gv[3] = hi.y;
                // (Gs is no part of the region the wave slices share: no wave still reads what these stores overwrite)
                double* dst = Gs + (ilv ? cpos(gi) * GS + cpos(gj) : gi * GS + gj);
                const int ds = ilv ? 2 : 1;
#pragma unroll
                for (int k = 0; k < 4; ++k) dst[k * ds] = gv[k];
            } else {
            double* dst = Gs + gi * GS + gj;
            dst[0] = lo.x;
            dst[1] = lo.y;
            dst[2] = hi.x;
            dst[3] = hi.y;
            }
        }
        __syncthreads();
        if constexpr (GRAN) {
            if (G > 1 && flags[3]) return;
        }
        SWEEP_STAMP(3);
        // ---- 3a, 3b. deflation and convergence measure
        double off;
        bool any_null;
        if constexpr (RP) {
            // ONE interval between two barriers: every thread measures its four elements from its registers against the diagonal
            // in LDS (the terms of gram_offmax, each formed once by the thread that holds the element), lanes < JP test the
            // rows, and V is filled with the identity in the layout the Gram was written in (V and the second Gram buffer lie in
            // the region of the wave slices, which the barrier behind the exchange has just released)
            const int gi = tid >> 3, gj = 4 * (tid & 7);
            double m = 0.0;
            if (gi < gj + 3) {
                const double gii = Gs[(ilv ? cpos(gi) : gi) * (GS + 1)];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = gj + k;
                    if (gi < j) {
                        const double den = gii * Gs[(ilv ? cpos(j) : j) * (GS + 1)];
                        if (den > 0.0) m = fmax(m, fabs(gv[k]) * rsqrt(den));
                    }
                }
            }
            m = wave_max(m);
            if (lane == 0) red[wave] = m;
            if (tid < JP) {
                double g = Gs[(ilv ? cpos(tid) : tid) * (GS + 1)];
                if constexpr (CPLX) g = fmax(g, Gs[(tid ^ 1) * (GS + 1)]); // (a complex row is null or not as a whole)
                const int z = (g > 0.0 && g <= mt.thr2) ? 1 : 0;
                zrow[tid] = z;
                perm[tid] = tid;
                if (z) flags[0] = 1;
            }
            if constexpr (!CPLX) {
                for (int e = tid; e < JP * VS; e += NT) {
                    const int k = e / VS;
                    Va[e] = ((ilv ? cpos(k) : k) == (e % VS)) ? 1.0 : 0.0;
                }
            }
            __syncthreads();
            off = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
            any_null = flags[0] != 0;
            if (any_null) {
                // rare: the measure is taken on the Gram with the null rows zeroed, in natural layout (no cross-only solve)
#pragma unroll
                for (int k = 0; k < 4; ++k) Gs[gi * GS + gj + k] = (zrow[gi] || zrow[gj + k]) ? 0.0 : gv[k];
                if (ilv)
                    for (int e = tid; e < JP * VS; e += NT) Va[e] = ((e / VS) == (e % VS)) ? 1.0 : 0.0;
                __syncthreads();
                off = gram_offmax(Gs, red, tid);
            }
        } else {
        // ---- 3a. deflation
        if (tid == 0) flags[0] = 0;
        __syncthreads();
        if (tid < JP) {
            double g = Gs[tid * GS + tid];
            if constexpr (CPLX) g = fmax(g, Gs[(tid ^ 1) * GS + (tid ^ 1)]); // (a complex row is null or not as a whole)
            const int z = (g > 0.0 && g <= mt.thr2) ? 1 : 0;
            zrow[tid] = z;
            perm[tid] = tid;
            if (z) flags[0] = 1;
        }
        __syncthreads();
        any_null = flags[0] != 0;
        if (any_null) {
            for (int e = tid; e < JP * JP; e += NT) {
                const int i = e / JP, j = e % JP;
                if (zrow[i] || zrow[j]) Gs[i * GS + j] = 0.0;
            }
            __syncthreads();
        }
        // ---- 3b. convergence measure
        off = gram_offmax(Gs, red, tid);
        }
        if (part == 0 && tid == 0) atomicMax(offmax_bits + (size_t)sw * sc.n_mats + mt.mat, (unsigned long long)__double_as_longlong(off));
        const bool skip = off <= mt.tol && !any_null; // pair already orthogonal: rows stay as they are
        if (!skip) {
            double* Ga = Gs;
            double* Gb = G2;
            double* Vc = Va;
            double* Vn = Vb;
            bool pos_is_interleaved = false; // cross-only solve: position 2k holds row k of block P, 2k + 1 row k of block Q
            const bool cross = cross_terms && !any_null; // (the same in every part)
            if constexpr (CPLX) {
                // ---- 3c'. rows are the interleaved embedding of complex rows: structure-preserving pivot solve by wave 0
                //           (work arrays in G2, rotations in Vb, result M(Q_c) in Va, eigenvalues on the diagonal of Gs)
                if (tid < 64) hermitian_pivot_solve(Gs, G2, Vb, Va, Gs, max_inner, tid, 0.25 * mt.tol * mt.tol, cross);
                __syncthreads();
            } else {
            // ---- 3c. eigensolve in position space (see the head of this section)
            pos_is_interleaved = cross;
            if constexpr (RP) {
                // (the Gram lies in Gs in the layout of the solve and V holds its identity: the first step follows at once)
            } else {
            if (cross) {
                for (int e = tid; e < JP * JP; e += NT) {
                    const int i = e / JP, j = e % JP;
                    Gb[cpos(i) * GS + cpos(j)] = Ga[i * GS + j];
                }
                for (int e = tid; e < JP * VS; e += NT) Va[e] = (cpos(e / VS) == (e % VS)) ? 1.0 : 0.0;
                double* t = Ga;
                Ga = Gb;
                Gb = t;
            } else
                for (int e = tid; e < JP * VS; e += NT) Va[e] = ((e / VS) == (e % VS)) ? 1.0 : 0.0;
            __syncthreads();
            }
            {
                const int pr = tid >> 4, pc = tid & 15;
                const int r0 = 2 * pr, c0 = 2 * pc;
                // destinations of a step: the ring of all 32 positions, or (cross) even positions stay and odd ones move on by one pair
                const int dr0 = cross ? r0 : ring_next(r0), dr1 = cross ? ((r0 + 3) & (JP - 1)) : ring_next(r0 + 1);
                const int dc0 = cross ? c0 : ring_next(c0), dc1 = cross ? ((c0 + 3) & (JP - 1)) : ring_next(c0 + 1);
                const int n_steps = cross ? JB : JP - 1;
                for (int sweep = 0; sweep < (off <= mt.tol ? 0 : max_inner); ++sweep) {
                    for (int r = 0; r < n_steps; ++r) {
                        const d2 g0 = *reinterpret_cast<const d2*>(Ga + r0 * GS + c0);
                        const d2 g1 = *reinterpret_cast<const d2*>(Ga + (r0 + 1) * GS + c0);
                        const d2 ac = *reinterpret_cast<const d2*>(Ga + c0 * GS + c0);
                        const double dc = Ga[(c0 + 1) * GS + c0 + 1];
                        const d2 v0 = *reinterpret_cast<const d2*>(Vc + r0 * VS + c0);
                        const d2 v1 = *reinterpret_cast<const d2*>(Vc + (r0 + 1) * VS + c0);
                        // ONE rotation chain per thread (its column pair; the eigensolver is bound by the f64 instruction count of
                        // its single wave per SIMD: scripts/probes/eig_step_probe.hip, 1196 -> 935 cycles per step); the row
                        // pair's rotation is the one lane pc == pr of the same 16-lane row has just derived
                        double c1, s1, c2, s2;
                        jacobi_rot_bf(ac.x, dc, ac.y, c2, s2, 0.25 * mt.tol * mt.tol);
                        const int rsrc = (lane & 48) | pr;
                        c1 = __shfl(c2, rsrc);
                        s1 = __shfl(s2, rsrc);
                        const double hik = c1 * g0.x - s1 * g1.x, hil = c1 * g0.y - s1 * g1.y;
                        const double hjk = s1 * g0.x + c1 * g1.x, hjl = s1 * g0.y + c1 * g1.y;
                        double nik = c2 * hik - s2 * hil, nil = s2 * hik + c2 * hil;
                        double njk = c2 * hjk - s2 * hjl, njl = s2 * hjk + c2 * hjl;
                        if (pr == pc) {
                            nil = 0.0;
                            njk = 0.0;
                        }
                        Gb[dr0 * GS + dc0] = nik;
                        Gb[dr0 * GS + dc1] = nil;
                        Gb[dr1 * GS + dc0] = njk;
                        Gb[dr1 * GS + dc1] = njl;
                        Vn[r0 * VS + dc0] = c2 * v0.x - s2 * v0.y;
                        Vn[r0 * VS + dc1] = s2 * v0.x + c2 * v0.y;
                        Vn[(r0 + 1) * VS + dc0] = c2 * v1.x - s2 * v1.y;
                        Vn[(r0 + 1) * VS + dc1] = s2 * v1.x + c2 * v1.y;
                        __syncthreads();
                        double* t = Ga;
                        Ga = Gb;
                        Gb = t;
                        t = Vc;
                        Vc = Vn;
                        Vn = t;
                    }
                    if (sweep + 1 < max_inner) {
                        const double off_in = gram_offmax(Ga, red, tid);
                        if (off_in <= 0.25 * mt.tol) break;
                    }
                }
            }
            } // (real pivot solve)
            auto row_at = [&](int p) { return pos_is_interleaved ? cidx(p) : p; }; // the row of the pair that sits at position p
            if constexpr (RP) {
                // (both solves end behind a barrier of their own)
                SWEEP_STAMP(4);
                if (off > mt.tol) {
                    // rank of every row by descending norm (padding rows last) on all four waves: wave w ranks the positions
                    // 8 w .. 8 w + 7, eight lanes per position compare its key with four of the 32 keys each, the partial
                    // ranks meet in the 8-lane group.  The lane that writes perm also forms zout.
                    const int li = 8 * wave + (lane >> 3), ch = lane & 7;
                    auto key = [&](int p) { return xrow(row_at(p), P, Q) < mt.nv ? Ga[p * GS + p] : -1.0e300; };
                    const double g = key(li);
                    int rk = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = 4 * ch + k;
                        const double gj = key(j);
                        rk += (gj > g || (gj == g && j < li)) ? 1 : 0;
                    }
                    rk += __shfl_xor(rk, 1);
                    rk += __shfl_xor(rk, 2);
                    rk += __shfl_xor(rk, 4);
                    if (ch == 0) {
                        perm[rk] = li;
                        zout[rk] = zrow[row_at(li)];
                    }
                } else if (tid < JP)
                    zout[tid] = zrow[row_at(tid)]; // (perm is the identity of step 3a)
                __syncthreads();
                SWEEP_STAMP(5);
            } else {
            __syncthreads();
            SWEEP_STAMP(4);
            if (off > mt.tol && tid < 64) {
                // rank of every row by descending norm (padding rows last): lane i of wave 0 holds key i and takes the other
                // keys from the lanes by v_readlane (a scalar broadcast) instead of 32 dependent LDS reads: 1.6 -> 0.4 us
                const int li = lane & (JP - 1);
                const int li_idx = row_at(li);
                const double g = xrow(li_idx, P, Q) < mt.nv ? Ga[li * GS + li] : -1.0e300;
                const int glo = __double2loint(g), ghi = __double2hiint(g);
                int rk = 0;
#pragma unroll
                for (int j = 0; j < JP; ++j) {
                    const double gj = __hiloint2double(__builtin_amdgcn_readlane(ghi, j), __builtin_amdgcn_readlane(glo, j));
                    rk += (gj > g || (gj == g && j < li)) ? 1 : 0;
                }
                if (lane < JP) perm[rk] = lane;
            }
            __syncthreads();
            // ---- 4. X <- Qm^T X on the own chunks, stored write-through for the next owner
            for (int e = tid; e < JP * JP; e += NT) {
                const int k = e / JP, m = e % JP;
                Qs[k * QS + m] = Vc[k * VS + perm[m]];
            }
            if (tid < JP) zout[tid] = zrow[row_at(perm[tid])]; // (perm holds positions; zrow is per row of the pair)
            __syncthreads();
            SWEEP_STAMP(5);
            }
            if (ct > nW) { // J is updated in this round: its rows must have been through every earlier round's update
                if (tid == 0) {
                    flags[1] = spin_pair<RORD>(readyJ + (size_t)P * G + part, readyJ + (size_t)Q * G + part, (unsigned int)ground, sc.err) ? 1 : 0;
                }
                __syncthreads();
                if (!flags[1]) return;
#pragma unroll
                for (int c = 0; c < SW_PRE; ++c) {
                    if (c >= pre_limit && c < ct) {
#pragma unroll
                        for (int kk = 0; kk < JP / 4; ++kk) xpre[c][kk] = chunk_load(c, 4 * kk + ukq);
                    }
                }
            }
            if (ct > 0) {
                // ---- 4. X <- Qm^T X on the own chunks, stored write-through for the next owner.  Qm[k][m] = V[k][perm[m]]:
                //         RP reads the MFMA operands from V through perm, the copy Qs is built only where a deferred J
                //         update will read it, behind the update (below)
                const double* ap0 = RP ? Vc + (lane >> 4) * VS + perm[lane & 15] : Qs + (lane >> 4) * QS + (lane & 15);
                const double* ap1 = RP ? Vc + (lane >> 4) * VS + perm[16 + (lane & 15)] : ap0 + 16;
                constexpr int AS = RP ? VS : QS;
                double a0[JP / 4], a1[JP / 4];
#pragma unroll
                for (int kk = 0; kk < JP / 4; ++kk) {
                    a0[kk] = ap0[kk * 4 * AS];
                    a1[kk] = ap1[kk * 4 * AS];
                }
                int zr[2][4];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) zr[i][q] = zout[i * 16 + (lane >> 4) + 4 * q];
                auto apply = [&](int c, const double (&xb)[JP / 4]) {
                    d4 acc[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
                    for (int kk = 0; kk < JP / 4; ++kk) {
                        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[kk], xb[kk], acc[0], 0, 0, 0);
                        acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[kk], xb[kk], acc[1], 0, 0, 0);
                    }
                    const bool zero_null = c < nW;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int row = i * 16 + (lane >> 4) + 4 * q;
                            bool in_w;
                            const unsigned int o = chunk_off(c, row, in_w);
                            Q8 v;
                            v.d = (zero_null && zr[i][q]) ? 0.0 : acc[i][q];
                            if (in_w) __builtin_amdgcn_raw_buffer_store_b64(v.u, rsW, o, 0, 16);
                            else __builtin_amdgcn_raw_buffer_store_b64(v.u, rsJ, o, 0, 16);
                        }
                };
#pragma unroll
                for (int c = 0; c < SW_PRE; ++c)
                    if (c < ct) apply(c, xpre[c]);
                if (ct > SW_PRE) {
                    double xb[JP / 4], xn[JP / 4];
#pragma unroll
                    for (int kk = 0; kk < JP / 4; ++kk) xb[kk] = chunk_load(SW_PRE, 4 * kk + ukq);
                    if constexpr (RORD) {
                        // as in the Gram loop: the buffers swap roles and the test for a next chunk is hoisted, so that the
                        // MFMAs of a chunk wait with a counted vmcnt and the next chunk's loads stay in flight behind them
                        auto fetch = [&](double (&x)[JP / 4], int c) {
#pragma unroll
                            for (int kk = 0; kk < JP / 4; ++kk) x[kk] = chunk_load(c, 4 * kk + ukq);
                        };
                        for (int c = SW_PRE;;) {
                            if (c + 1 < ct) {
                                fetch(xn, c + 1);
                                apply(c, xb);
                            } else {
                                apply(c, xb);
                                break;
                            }
                            ++c;
                            if (c + 1 < ct) {
                                fetch(xb, c + 1);
                                apply(c, xn);
                            } else {
                                apply(c, xn);
                                break;
                            }
                            ++c;
                        }
                    } else
                    for (int c = SW_PRE; c < ct; ++c) {
                        if (c + 1 < ct) {
#pragma unroll
                            for (int kk = 0; kk < JP / 4; ++kk) xn[kk] = chunk_load(c + 1, 4 * kk + ukq);
                        }
                        apply(c, xb);
#pragma unroll
                        for (int kk = 0; kk < JP / 4; ++kk) xb[kk] = xn[kk];
                    }
                }
            }
            if constexpr (RP) {
                // Qm for the deferred J update of the next round, off the chain: the W stores are on their way, the barrier
                // of step 5 makes it visible (nobody else reads Qs: this round's J chunks took their operands above)
                if (defer) {
                    for (int e = tid; e < JP * JP; e += NT) {
                        const int k = e / JP, m = e % JP;
                        Qs[k * QS + m] = Vc[k * VS + perm[m]];
                    }
                }
            }
        }
        if (defer && !skip) { // the J half of this update waits for the next round's exchange
            pendP = P;
            pendQ = Q;
            pend_ground = ground;
        }
        // ---- 5. hand the two row blocks on: every storing wave drains, barrier, ONE lane publishes
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            if (skip && nJ > 0) { // (J untouched, but it may only be passed on once the earlier rounds' updates are in)
                if constexpr (RORD) (void)spin_until2(readyJ + (size_t)P * G + part, readyJ + (size_t)Q * G + part, (unsigned int)ground, sc.err);
                else {
                    (void)spin_until(readyJ + (size_t)P * G + part, (unsigned int)ground, sc.err);
                    (void)spin_until(readyJ + (size_t)Q * G + part, (unsigned int)ground, sc.err);
                }
            }
            __hip_atomic_store(ready + (size_t)P * G + part, (unsigned int)(ground + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ready + (size_t)Q * G + part, (unsigned int)(ground + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!(defer && !skip)) { // (J is up to date: updated above, or the pair was skipped)
                __hip_atomic_store(readyJ + (size_t)P * G + part, (unsigned int)(ground + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(readyJ + (size_t)Q * G + part, (unsigned int)(ground + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // one-launch form: this entry's share of the sweep is done (its off-norm contributions -- atomics of this very
            // lane, completed: they return a value the drain above waited for -- are in)
            if (n_sw > 1 && round == mt.nb - 2) __hip_atomic_fetch_add(sc.arrive + mt.mat, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        SWEEP_STAMP(6);
    }
    } // entries x rounds
    if (n_sw == 1) break;
    // ---- end of a sweep, one-launch form: the host's convergence test (jacobi_sweep_done), on the device.  Every entry
    //      of a matrix sees the same off-norms, hence takes the same decision; an entry waits until all entries of its
    //      matrix have finished the sweep, workgroups whose entries have all converged leave.
    __syncthreads();
    if (tid == 0) {
        int all = 1, ok = 1;
        for (int ent = went.x; ent < went.y && ok; ++ent) {
            if (edone[ent - went.x]) continue;
            const int2 wm = sc.wgmap[ent];
            const RPair mt = pairs[wm.x];
            const unsigned int entries = (unsigned int)(mt.nb / 2) * (unsigned int)mt.pad[0];
            if (!spin_until<32>(sc.arrive + mt.mat, entries * (unsigned int)(sw + 1), sc.err)) { // (every workgroup of the matrix polls this word)
                ok = 0;
                break;
            }
            const double off = __longlong_as_double((long long)__hip_atomic_load(offmax_bits + (size_t)sw * sc.n_mats + mt.mat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const double prev = sw ? __longlong_as_double((long long)__hip_atomic_load(offmax_bits + (size_t)(sw - 1) * sc.n_mats + mt.mat,
                                                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                                   : 1e300;
            if (jacobi_sweep_done(off, prev, mt.tol, sw + 1)) { // (the rule counts sweeps from one)
                edone[ent - went.x] = 1;
                if (mt.slot == 0 && wm.y == 0) sc.nsw[mt.mat] = sw + 1;
            } else all = 0;
        }
        flags[1] = ok;
        flags[2] = all;
    }
    __syncthreads();
    if (!flags[1] || flags[2]) return;
    } // sweeps
#undef SWEEP_STAMP
}

// ================================================================================================
// Host driver.  One sweep over the list is six steps (see jacobi_orthogonalise): work list, plan, scratch, launch,
// read-back, verdicts.

struct JSwitches {       // CYB_JACOBI_* (DESIGN.md section 7), read once per process
    bool no_sweep;       // NOSWEEP: every list takes the split route (the test hook of the fallback)
    bool per_sweep;      // PERSWEEP: a launch per sweep for every list
    bool one_launch_all; // ONELAUNCH: one launch for all sweeps of every list
    bool trace;          // TRACE: print every matrix's off-norm after every sweep
    bool stamps;         // STAMPS: phase times of one round of the sweep kernel
    bool no_predict;     // NOPREDICT: the last sweep is never predicted
    bool gran_exchange;  // EXCHANGE=0: the partial Grams of the sweep kernel travel by stores, drain, ticket and poll (same sums
                         // in the same order: bit-identical results); default: as tagged granules
    bool round_order;    // ROUND_ORDER=0: the issue order a round had before (same arithmetic, same protocol: bit-identical results)
    bool round_passes;   // ROUND_PASSES=0: the LDS passes and barriers around the pivot solve as they were before they were folded
                         // (same arithmetic: bit-identical results); the folded form needs the default order and exchange
    bool no_defer_j;     // NODEFERJ: the sweep kernel updates J at once
    bool cross_small;    // CROSS_SMALL: cross-only pivot solves for lists of small matrices too
    int g;               // G: parts per pair (0: chosen by plan_parts / per split round)
    int inner;           // INNER: inner sweeps per pivot solve (0: chosen per list)
    int cross;           // CROSS: SScratch::cross_every
    int cross_min_nb;    // CROSS_MINNB: SScratch::cross_min_nb
};
const JSwitches& switches()
{
    static const JSwitches s = [] {
        auto on = [](const char* name) { return getenv(name) != nullptr; };
        auto num = [](const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; };
        JSwitches w;
        w.no_sweep = on("CYB_JACOBI_NOSWEEP");
        w.per_sweep = on("CYB_JACOBI_PERSWEEP");
        w.one_launch_all = on("CYB_JACOBI_ONELAUNCH");
        w.trace = on("CYB_JACOBI_TRACE");
        w.stamps = on("CYB_JACOBI_STAMPS");
        w.no_predict = on("CYB_JACOBI_NOPREDICT");
        w.gran_exchange = num("CYB_JACOBI_EXCHANGE", 1) != 0;
        w.round_order = num("CYB_JACOBI_ROUND_ORDER", 1) != 0;
        w.round_passes = num("CYB_JACOBI_ROUND_PASSES", 1) != 0 && w.round_order && w.gran_exchange;
        w.no_defer_j = on("CYB_JACOBI_NODEFERJ");
        w.cross_small = on("CYB_JACOBI_CROSS_SMALL");
        w.g = num("CYB_JACOBI_G", 0);
        w.inner = num("CYB_JACOBI_INNER", 0);
        w.cross = num("CYB_JACOBI_CROSS", -1);
        w.cross_min_nb = num("CYB_JACOBI_CROSS_MINNB", 0);
        return w;
    }();
    return s;
}

struct SweepCall {   // what stays the same over the sweeps of one call
    int n;           // matrices of the call (active or not: the convergence words are indexed by matrix)
    int n_sw_dev;    // sweeps the one-launch form may run on the device (1: a launch per sweep)
    size_t w_off;    // off-norm words: n * n_sw_dev
    size_t b_off;    // bytes of the convergence words; the error word follows
    bool cplx;
};

// ---- step 1: work list
struct SweepList {
    std::vector<int> order;    // active matrices, more row blocks first (late rounds of the split route use a prefix of the grid)
    std::vector<JWork> wl;     // one item per block pair: (matrix, pair slot)
    std::vector<PlanMat> pm;   // [position in order] what the plan looks at
    int max_nb = 0;
    bool any_j = false;
    bool big_ok = true;        // every W and J lies within the 32-bit buffer offsets of the sweep kernel
};
SweepList build_work_list(const std::vector<JMat>& h_mats, const std::vector<int>& active)
{
    SweepList l;
    l.order = active;
    std::stable_sort(l.order.begin(), l.order.end(), [&](int a, int b) { return h_mats[(size_t)a].nb > h_mats[(size_t)b].nb; });
    for (int m : l.order) {
        const JMat& jm = h_mats[(size_t)m];
        l.max_nb = std::max(l.max_nb, jm.nb);
        for (int k = 0; k < jm.nb / 2; ++k) l.wl.push_back(JWork{m, k});
        l.pm.push_back(PlanMat{jm.nb, jm.nvp, jm.lenp, jm.J != nullptr || jm.rec_j != 0});
        l.any_j = l.any_j || jm.J != nullptr;
        l.big_ok = l.big_ok && (size_t)jm.nvp * (size_t)std::max(jm.lenp, jm.nvp) * 8 < ((size_t)1 << 31);
    }
    return l;
}

// ---- step 3: scratch of both routes in one grow-only workspace:
//      [zeroed block (SweepLayout) | granule regions | Gram partials | hand-off of the split route]
struct SweepScratch {
    void* base = nullptr;         // the zeroed block starts here: ONE fill per sweep, issued by whichever route runs it
    size_t zero_bytes;            // ... and is this long (the sweep kernel adds the granule regions of its parts)
    unsigned long long* d_off;    // convergence words: off-norm bits per matrix (one-launch form: see jacobi_orthogonalise)
    unsigned int* d_err;          // set when a bounded wait ran out
    unsigned int* d_ready;        // [one ticket per pair | ready counters of W | ready counters of J]
    unsigned long long* d_gran;
    double* gpart;                // (a sweep runs one route or the other)
    JScratch split;
    size_t split_cnt_bytes;
};
int carve_scratch(cyb_ctx_t ctx, const SweepLayout& L, size_t b_off, SweepScratch& s)
{
    const size_t np = L.np;
    const size_t b_gpart = sizeof(double) * np * RGMAX * JP * JP, b_q = sizeof(double) * np * JP * JP;
    const size_t b_z = sizeof(int32_t) * np * JP, b_f = (sizeof(int32_t) * np + 15) / 16 * 16, b_c = (sizeof(unsigned int) * np + 15) / 16 * 16;
    void* wsp = nullptr;
    const int status = ctx->workspace(L.zero_bytes + L.gran_reserved + 2 * b_gpart + 2 * (b_q + b_z + b_f) + b_c + 1024, &wsp, 2);
    if (status != CYB_OK) return status;
    char* bp = static_cast<char*>(wsp);
    s.base = wsp;
    s.zero_bytes = L.zero_bytes;
    s.d_off = reinterpret_cast<unsigned long long*>(bp);
    s.d_err = reinterpret_cast<unsigned int*>(bp + b_off);
    s.d_ready = reinterpret_cast<unsigned int*>(bp + b_off + 16);
    s.d_gran = reinterpret_cast<unsigned long long*>(bp + L.zero_bytes);
    bp += L.zero_bytes + L.gran_reserved;
    s.gpart = reinterpret_cast<double*>(bp);
    bp += 2 * b_gpart;
    s.split.gpart = s.gpart;
    for (int h = 0; h < 2; ++h) {
        s.split.qout[h] = reinterpret_cast<double*>(bp);
        bp += b_q;
    }
    for (int h = 0; h < 2; ++h) {
        s.split.zout[h] = reinterpret_cast<int32_t*>(bp);
        bp += b_z;
    }
    for (int h = 0; h < 2; ++h) {
        s.split.flag[h] = reinterpret_cast<int32_t*>(bp);
        bp += b_f;
    }
    s.split.cnt = reinterpret_cast<unsigned int*>(bp);
    s.split_cnt_bytes = b_c;
    return CYB_OK;
}

// ---- step 4, sweep kernel.  Its descriptors ([pair descriptors | entry map | workgroup map], ONE upload) stay on the device
//      while the active set and its parts are those of the previous sweep and the ring slot is still alive.
struct ImageCache {
    std::vector<int> order, G;
    uint64_t at = 0;
    void* img = nullptr;
};
int descriptor_image(cyb_ctx_t ctx, ImageCache& cache, const std::vector<JMat>& h_mats, const SweepList& list, const SweepPlan& plan)
{
    uint64_t& cached_at = cache.at; // n_uploads after the upload that filled the image (tests/test_call_sequences.py: the ring's contract)
    if (cache.img && list.order == cache.order && plan.G == cache.G && ctx->n_uploads - cached_at < (uint64_t)cyb_ctx_s::kSlots / 2 - 1)
        return CYB_OK;
    const SweepLayout& L = plan.layout;
    std::vector<char> img(L.image_bytes);
    RPair* rp = reinterpret_cast<RPair*>(img.data());
    int2* wgmap = reinterpret_cast<int2*>(img.data() + L.map_off);
    size_t k = 0, e = 0;
    for (size_t i = 0; i < list.order.size(); ++i) {
        const JMat& jm = h_mats[(size_t)list.order[i]];
        for (int slot = 0; slot < jm.nb / 2; ++slot, ++k) {
            RPair& q = rp[k];
            q.W = jm.W;
            q.J = jm.J;
            q.tol = jm.tol;
            q.thr2 = jm.thr2;
            q.nvp = jm.nvp;
            q.lenp = jm.lenp;
            q.nb = jm.nb;
            q.nv = jm.nv;
            q.mat = list.order[i];
            q.slot = slot;
            q.pad[0] = plan.G[i];
            q.pad[1] = L.flag_base[i];
            for (int g = 0; g < plan.G[i]; ++g) wgmap[e++] = make_int2((int)k, g);
        }
    }
    if (!plan.share.ranges.empty()) memcpy(img.data() + L.ent_off, plan.share.ranges.data(), sizeof(PlanRange) * plan.share.ranges.size());
    const int status = ctx->upload(img.data(), img.size(), &cache.img);
    if (status != CYB_OK) return status;
    cache.order = list.order;
    cache.G = plan.G;
    cached_at = ctx->n_uploads;
    return CYB_OK;
}

typedef void (*sweep_fn_t)(const RPair*, int, unsigned long long*, SScratch);
int sweep_kernel_for(bool cplx, sweep_fn_t& fn)
{
    static const sweep_fn_t sweep_fns[2][2][2] = { // [CPLX][RORD][GRAN], passes around the pivot solve as before
        {{jacobi_sweep_kernel<false, false, false, false>, jacobi_sweep_kernel<false, false, true, false>},
         {jacobi_sweep_kernel<false, true, false, false>, jacobi_sweep_kernel<false, true, true, false>}},
        {{jacobi_sweep_kernel<true, false, false, false>, jacobi_sweep_kernel<true, false, true, false>},
         {jacobi_sweep_kernel<true, true, false, false>, jacobi_sweep_kernel<true, true, true, false>}}};
    static const sweep_fn_t sweep_fns_rp[2] = {jacobi_sweep_kernel<false, true, true, true>, jacobi_sweep_kernel<true, true, true, true>}; // [CPLX], folded
    const JSwitches& sw = switches();
    static const sweep_fn_t sweep_fn[2] = {sw.round_passes ? sweep_fns_rp[0] : sweep_fns[0][sw.round_order ? 1 : 0][sw.gran_exchange ? 1 : 0],
                                           sw.round_passes ? sweep_fns_rp[1] : sweep_fns[1][sw.round_order ? 1 : 0][sw.gran_exchange ? 1 : 0]};
    static bool attr_set = false;
    if (!attr_set) {
        for (int c = 0; c < 2; ++c)
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(sweep_fn[c]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)SWEEP_LDS_BYTES) != hipSuccess) {
                set_error("jacobi: cannot reserve %zu bytes of LDS for the sweep kernel", SWEEP_LDS_BYTES);
                return CYB_ERR_HIP;
            }
        attr_set = true;
    }
    fn = sweep_fn[cplx ? 1 : 0];
    return CYB_OK;
}

// CYB_JACOBI_STAMPS: phase times of round `stamp_round` for the workgroups of the matrix with the most blocks (the first
// of the work list: its entries are the first nb / 2 * G of the launch)
void print_sweep_stamps(hipStream_t st, const unsigned long long* d_stamps, const SweepList& list, const SweepPlan& plan, int sweep, int stamp_round)
{
    const size_t entries = plan.layout.entries;
    std::vector<unsigned long long> hs(8 * entries);
    if (hipMemcpyAsync(hs.data(), d_stamps, sizeof(unsigned long long) * hs.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return;
    double acc[6] = {0, 0, 0, 0, 0, 0}, passes = 0;
    const int cntw = list.pm[0].nb / 2 * plan.G[0];
    const bool swept = switches().gran_exchange && plan.G[0] > 1; // (slot 7: granule passes of wave 0)
    for (size_t b = 0; b < (size_t)cntw; ++b) {
        for (int k = 0; k < 6; ++k) acc[k] += (double)(hs[8 * b + k + 1] - hs[8 * b + k]) * 0.01;
        if (swept) passes += (double)hs[8 * b + 7];
    }
    if (cntw)
        fprintf(stderr, "[jacobi sweep stamps] sweep %d round %d, largest matrix (G=%d, %d workgroups of %zu): wait %.2f load+gram %.2f "
                        "exch %.2f defl+eig %.2f sort %.2f upd+publish %.2f us, granule passes %.1f\n",
                sweep, stamp_round, plan.G[0], cntw, entries, acc[0] / cntw, acc[1] / cntw, acc[2] / cntw, acc[3] / cntw, acc[4] / cntw,
                acc[5] / cntw, passes / cntw);
}

// Every pair of every matrix gets its workgroups for the whole sweep.  one_launch: this launch runs every sweep of the call.
int launch_sweep(cyb_ctx_t ctx, const std::vector<JMat>& h_mats, const SweepList& list, const SweepPlan& plan, const SweepScratch& s,
                 ImageCache& cache, const SweepCall& call, int sweep, int max_inner, bool& one_launch)
{
    const JSwitches& sw = switches();
    const SweepLayout& L = plan.layout;
    hipStream_t st = ctx->stream;
    int status = descriptor_image(ctx, cache, h_mats, list, plan);
    if (status != CYB_OK) return status;
    sweep_fn_t fn = nullptr;
    status = sweep_kernel_for(call.cplx, fn);
    if (status != CYB_OK) return status;
    const std::vector<PlanRange>& ranges = plan.share.ranges;
    static unsigned long long* d_stamps = nullptr; // diagnostic runs only: 2048 workgroups x 8 stamps
    if (sw.stamps && !d_stamps && hipMalloc(reinterpret_cast<void**>(&d_stamps), sizeof(unsigned long long) * 8 * 2048) != hipSuccess) d_stamps = nullptr;
    SScratch ss;
    ss.gpart = s.gpart;
    ss.ticket = s.d_ready;                   // [0, np): tickets; behind them the ready counters (flag_base offsets)
    ss.ready = s.d_ready;
    ss.readyJ = s.d_ready + L.ready_reserved; // (same offsets, second array)
    ss.defer_j = sw.no_defer_j ? 0 : 1;
    // (lists of small matrices run three inner sweeps per pivot solve: cross-only there is opt-in, CYB_JACOBI_CROSS_SMALL=1)
    ss.cross_every = (max_inner == 1 || sw.cross_small) ? sw.cross : 0;
    ss.cross_min_nb = sw.cross_min_nb;
    ss.err = s.d_err;
    ss.wgmap = reinterpret_cast<const int2*>(static_cast<char*>(cache.img) + L.map_off);
    ss.wgent = ranges.empty() ? nullptr : reinterpret_cast<const int2*>(static_cast<char*>(cache.img) + L.ent_off);
    ss.stamps = ranges.empty() ? d_stamps : nullptr;
    ss.stamp_round = std::min(3, list.max_nb - 2);
    size_t max_ent = 1;
    for (const PlanRange& we : ranges) max_ent = std::max(max_ent, (size_t)(we.end - we.begin));
    one_launch = call.n_sw_dev > 1 && sweep == 1 && max_ent <= (size_t)SW_MAX_ENT;
    ss.n_sweeps = one_launch ? call.n_sw_dev : 1;
    ss.n_mats = call.n;
    ss.arrive = reinterpret_cast<unsigned int*>(s.d_off + call.w_off);
    ss.nsw = reinterpret_cast<int*>(ss.arrive + call.n);
    ss.gran = s.d_gran;
    ss.gran_np = (int)L.np;
    if (L.gran_used > L.gran_reserved) {
        set_error("jacobi: %zu bytes of granule regions exceed the %zu reserved", L.gran_used, L.gran_reserved);
        return CYB_ERR_INVALID;
    }
    if (hipMemsetAsync(s.base, 0, s.zero_bytes + L.gran_used, st) != hipSuccess) return CYB_ERR_HIP;
    const size_t n_wg = ranges.empty() ? L.entries : ranges.size();
    hipLaunchKernelGGL(fn, dim3((unsigned)n_wg), dim3(NT), SWEEP_LDS_BYTES, st, static_cast<const RPair*>(cache.img), max_inner, s.d_off, ss);
    if (ss.stamps && L.entries <= 2048) print_sweep_stamps(st, d_stamps, list, plan, sweep, ss.stamp_round);
    return CYB_OK;
}

// ---- step 4, fallback: every round of the sweep on the split route, all matrices in lockstep.  The J half of a round's
//      update is deferred: it rides along with the next round's Gram launch (nothing reads J before the end).
int launch_rounds_split(cyb_ctx_t ctx, const std::vector<JMat>& h_mats, const SweepList& list, const SweepScratch& s, int max_inner)
{
    hipStream_t st = ctx->stream;
    const JScratch& sc = s.split;
    const int g_env = switches().g;
    if (hipMemsetAsync(s.base, 0, s.zero_bytes, st) != hipSuccess) return CYB_ERR_HIP;
    void *d_mats_v = nullptr, *d_wl = nullptr;
    int status = ctx->upload(h_mats.data(), sizeof(JMat) * h_mats.size(), &d_mats_v);
    if (status == CYB_OK) status = ctx->upload(list.wl.data(), sizeof(JWork) * list.wl.size(), &d_wl);
    if (status != CYB_OK) return status;
    const JMat* d_mats = static_cast<const JMat*>(d_mats_v);
    if (hipMemsetAsync(sc.cnt, 0, s.split_cnt_bytes, st) != hipSuccess) return CYB_ERR_HIP;
    int pend_round = -1;   // round whose J half is still to be applied ...
    size_t pend_cnt = 0;   // ... for this many pairs
    for (int r = 0; r < list.max_nb - 1; ++r) {
        size_t cnt = 0; // grid = prefix of the work list holding matrices with nb - 1 > r
        for (int m : list.order) {
            if (h_mats[(size_t)m].nb - 1 > r) cnt += (size_t)h_mats[(size_t)m].nb / 2;
            else break;
        }
        if (cnt == 0) break;
        // spread every pair over enough workgroups to fill the chip (2 resident per CU for A, more for B)
        const int slots = 2 * ctx->n_cu;
        // measured (chi=4096 list): splitting the Gram further than 2 ways costs more in the partial
        // exchange than it saves (G = 1: 72.2, 2: 71.9, 4: 75.4, 8: 88.7 ms per batched SVD)
        int G = g_env > 0 ? g_env : ((size_t)2 * cnt <= (size_t)slots ? 2 : 1);
        G = std::min(G, RGMAX);
        // the update kernel holds 3 workgroups per CU: one full wave of workgroups, no tail
        const int U = (int)std::min<size_t>(16, std::max<size_t>(1, (size_t)(3 * ctx->n_cu) / cnt));
        const int buf = r & 1;
        const int n_gram = (int)(cnt * G);
        int UJ = 1;
        size_t n_jwg = 0;
        if (pend_round >= 0) { // the J half of the previous round rides along in the idle workgroup slots
            const long long free_slots = (long long)slots - (long long)n_gram;
            UJ = (int)std::max<long long>(1, std::min<long long>(8, free_slots / (long long)pend_cnt));
            n_jwg = pend_cnt * (size_t)UJ;
        }
        hipLaunchKernelGGL(jacobi_gram_kernel, dim3((unsigned)(n_gram + n_jwg)), dim3(NT), 0, st, d_mats,
                           static_cast<const JWork*>(d_wl), r, G, max_inner, s.d_off, sc, buf, n_gram, pend_round, UJ);
        const bool defer = list.any_j;
        hipLaunchKernelGGL(jacobi_update_kernel, dim3((unsigned)(cnt * U)), dim3(NT), 0, st, d_mats,
                           static_cast<const JWork*>(d_wl), r, U, sc, buf, 1, defer ? 0 : 1);
        pend_round = defer ? r : -1;
        pend_cnt = cnt;
    }
    if (pend_round >= 0) { // the J half of the last round: the work list changes with the sweep
        const int U = (int)std::min<size_t>(16, std::max<size_t>(1, (size_t)(3 * ctx->n_cu) / pend_cnt));
        hipLaunchKernelGGL(jacobi_update_kernel, dim3((unsigned)(pend_cnt * U)), dim3(NT), 0, st, d_mats,
                           static_cast<const JWork*>(d_wl), pend_round, U, sc, pend_round & 1, 0, 1);
    }
    return CYB_OK;
}

// ---- step 5: ONE read-back per sweep: [convergence words | error word]
int read_back(cyb_ctx_t ctx, const SweepScratch& s, std::vector<unsigned long long>& h_off, size_t b_off)
{
    if (ctx->d2h(h_off.data(), s.d_off, b_off + 16) != CYB_OK) {
        set_error("jacobi: reading the convergence flags failed: %s", hipGetErrorString(hipGetLastError()));
        return CYB_ERR_HIP;
    }
    unsigned int h_err = 0;
    memcpy(&h_err, reinterpret_cast<const char*>(h_off.data()) + b_off, sizeof(unsigned int));
    if (h_err) {
        set_error("jacobi round kernel: a workgroup waited more than a second for the Gram partials of its pair "
                  "(partner workgroup not resident?)");
        return CYB_ERR_HIP;
    }
    return CYB_OK;
}

// ---- step 6: which matrices are done after sweep `sweep` (one-based); the others stay in `active`
void sweep_verdicts(const std::vector<JMat>& h_mats, const std::vector<unsigned long long>& h_off, int sweep, std::vector<int>& active,
                    std::vector<double>& prev_off, std::vector<int32_t>& sweeps_out)
{
    const JSwitches& sw = switches();
    std::vector<int> still;
    for (int m : active) {
        const JMat& jm = h_mats[(size_t)m];
        double off;
        memcpy(&off, &h_off[(size_t)m], sizeof(double));
        if (sw.trace) fprintf(stderr, "[jacobi] sweep %2d mat %3d (nv=%d len=%d) off=%.3e tol=%.3e\n", sweep, m, jm.nv, jm.len, off, jm.tol);
        if (jacobi_sweep_done(off, prev_off[(size_t)m], jm.tol, sweep, !sw.no_predict)) sweeps_out[(size_t)m] = sweep;
        else still.push_back(m);
        prev_off[(size_t)m] = off;
    }
    active.swap(still);
}
// ... and after a launch that ran every sweep: matrices the device marked converged are done, the rest did not converge
void one_launch_verdicts(const std::vector<unsigned long long>& h_off, const SweepCall& call, std::vector<int>& active,
                         std::vector<int32_t>& sweeps_out)
{
    const int* h_nsw = reinterpret_cast<const int*>(reinterpret_cast<const unsigned int*>(h_off.data() + call.w_off) + call.n);
    std::vector<int> still;
    for (int m : active) {
        if (h_nsw[m] > 0) sweeps_out[(size_t)m] = h_nsw[m];
        else still.push_back(m);
    }
    active.swap(still);
}

} // namespace

int jacobi_orthogonalise(cyb_ctx_t ctx, const std::vector<JMat>& h_mats, int max_sweeps,
                         std::vector<int32_t>& sweeps_out, bool cplx)
{   // cplx: the rows are the interleaved real embedding of complex rows (structure-preserving pivot solve; sweep kernel only)
    const int n = (int)h_mats.size();
    sweeps_out.assign((size_t)n, 0);
    if (n == 0) return CYB_OK;
    const JSwitches& sw = switches();

    std::vector<int> active;
    for (int i = 0; i < n; ++i) {
        if (h_mats[(size_t)i].nv <= 1) sweeps_out[(size_t)i] = 0; // nothing to orthogonalise
        else active.push_back(i);
    }
    // convergence words of a sweep: [off-norm bits per matrix | error word], the head of the zeroed scratch block, so
    // that a sweep costs ONE memset before and ONE read-back after its kernel(s)
    // One launch for ALL sweeps (persistent sweep kernel, convergence test on the device): saves
    // the read-back, the host's turn-around and the launch of every sweep but the first (40-100 us each).  Correct (same
    // sweep counts, tests green) but NOT faster for large matrices: the chi=4096 list 34.0 against 34.2-34.4 ms per batched SVD, the toy DMRG
    // at chi=256 0.27-0.29 against 0.28-0.31 s per sweep (both inside the run-to-run spread), and a single rank-deficient 1442^2
    // block 29.9 against 28.9 ms -- its one kernel runs 15.7 ms where the ten per-sweep kernels sum to 14.5 ms (the sweep-end
    // wait of 192 workgroups on one word costs more than the launch boundary it replaces).  The control words of this form
    // are [off-norm bits per (sweep, matrix) | arrivals per matrix | sweeps per matrix].
    // Default therefore: lists of SMALL matrices only (at most 16 row blocks each -- the sectors of a DMRG bond around chi = 256:
    // few workgroups per matrix wait at a sweep's end, and the seven read-backs are a visible part of a 2 ms call; toy DMRG,
    // three runs each: 0.271 / 0.275 / 0.280 against 0.282 / 0.283 / 0.285 s per sweep).  CYB_JACOBI_ONELAUNCH=1: every list,
    // CYB_JACOBI_PERSWEEP=1: none.
    const bool one_launch_ok = !sw.per_sweep && !sw.trace && !sw.stamps && !sw.no_predict;
    int nb_max_all = 0;
    for (int i = 0; i < n; ++i) nb_max_all = std::max(nb_max_all, h_mats[(size_t)i].nb);
    SweepCall call;
    call.n = n;
    call.n_sw_dev = (one_launch_ok && (sw.one_launch_all || nb_max_all <= 16)) ? max_sweeps : 1;
    call.w_off = (size_t)n * (size_t)call.n_sw_dev;
    call.b_off = (sizeof(unsigned long long) * call.w_off + 2 * sizeof(unsigned int) * (size_t)n + 15) / 16 * 16;
    call.cplx = cplx;
    std::vector<unsigned long long> h_off(call.b_off / 8 + 2);
    const size_t sweep_slots = (size_t)SWEEP_WG_PER_CU * (size_t)ctx->n_cu; // resident workgroups the sweep kernel may use
    ImageCache cache;
    std::vector<double> prev_off((size_t)n, 1e300);
    bool one_launch_done = false;
    int status = CYB_OK;
    for (int sweep = 1; sweep <= max_sweeps && !active.empty(); ++sweep) {
        // 1. work list
        const SweepList list = build_work_list(h_mats, active);
        // inner Jacobi sweeps per pair visit: measurements and a numpy model agree that more than two
        // buy no outer sweeps, and one is fastest overall (measured: 81 vs 88 ms on the chi=4096 list)
        // ... except for batches of small matrices (at most 8 row blocks each: the DMRG regime around chi = 256), where a
        // round is all latency and an outer sweep costs a host read-back: three inner sweeps save outer sweeps there
        // (toy DMRG chi=256, eleven sweeps: 6.6-6.7 -> 6.3-6.6 s; the 13-block chi=1024 list, 23 row blocks: 11.6 -> 14.9 ms, so not there)
        const int max_inner = sw.inner > 0 ? sw.inner : (list.max_nb <= 8 ? 3 : 1);
        // 2. plan: parts per pair, shared workgroups, layout (arithmetic only; the scratch is sized from its layout)
        const SweepPlan plan = plan_sweep(list.pm, sweep_slots, sw.g, call.b_off + 16, sw.gran_exchange);
        // 3. scratch
        SweepScratch scratch;
        status = carve_scratch(ctx, plan.layout, call.b_off, scratch);
        if (status != CYB_OK) break;
        // 4. launch: the sweep kernel, or every round on the split route
        if (!sw.no_sweep && list.big_ok && plan.layout.fits) {
            status = launch_sweep(ctx, h_mats, list, plan, scratch, cache, call, sweep, max_inner, one_launch_done);
        } else if (cplx) {
            set_error("block-Jacobi on embedded complex rows needs the persistent sweep kernel (list too large for one launch)");
            status = CYB_ERR_UNSUPPORTED;
        } else {
            cache.img = nullptr; // (the uploads of the split route recycle the ring)
            status = launch_rounds_split(ctx, h_mats, list, scratch, max_inner);
        }
        if (status != CYB_OK) break;
        if (hipGetLastError() != hipSuccess) {
            set_error("jacobi round kernels: launch failed");
            status = CYB_ERR_HIP;
            break;
        }
        // 5. read back
        status = read_back(ctx, scratch, h_off, call.b_off);
        if (status != CYB_OK) break;
        // 6. verdicts
        if (one_launch_done) {
            one_launch_verdicts(h_off, call, active, sweeps_out);
            break;
        }
        sweep_verdicts(h_mats, h_off, sweep, active, prev_off, sweeps_out);
    }
    if (status != CYB_OK) return status;
    if (!active.empty()) {
        for (int m : active) sweeps_out[(size_t)m] = -1;
        set_error("block-Jacobi did not converge within %d sweeps for %zu matrices", max_sweeps, active.size());
        return CYB_ERR_NOCONV;
    }
    return CYB_OK;
}

} // namespace cyb

