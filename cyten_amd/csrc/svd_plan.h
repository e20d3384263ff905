// Plan of the QR-preconditioned SVD pipeline (svd_jacobi.hip: SvdPipeline and svd_batched_impl): the switches, where every
// piece of a call's workspace lies, which rows are deflated, which blocks take the second (LQ) step and which of those iterate
// without accumulating rotations, which column of Q2 completes which null row, and which blocks of a list go to the in-LDS
// kernel, the direct iteration or the pipeline.  All of it is host arithmetic on numbers the host already holds: the driver
// consumes it and tests/svd_plan.cpp walks it on the host.  No HIP in here; the CYB_SVD_* switches are read in svd_jacobi.hip
// and arrive as an SvdSwitches; the sizes blocked_qr.h decides arrive as an SvdAux.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <math.h>
#include <vector>

namespace cyb {

constexpr double kEps = 2.220446049250313e-16;

// Jacobi convergence threshold on |g_ij| / sqrt(g_ii g_jj) for vectors of length len
inline double jacobi_tol(int len) { return kEps * std::max(16.0, 4.0 * sqrt((double)len)); }

// ---- switches ---------------------------------------------------------------------------------------------------------------
// Every CYB_SVD_<NAME> environment switch, read once per process (svd_switches() in svd_jacobi.hip); the member initialisers
// are the defaults.  Flags are set by the presence of the variable, numbers by its value.
struct SvdSwitches {
    bool nolq = false;             // NOLQ: no block takes the LQ step (the plain iteration on R)
    bool lq_always = false;        // LQ_ALWAYS: every block with two surviving rows takes it
    int lq_skip_k = 128;           // LQ_SKIP_K, LQ_SKIP_RATIO: a full-rank block of at least this many rows whose row norms
    double lq_skip_ratio = 1e4;    //   of R lie within this ratio skips the LQ step (wants_lq)
    bool nojrec = false;           // NOJREC: the sweeps accumulate the rotations everywhere (the A/B switch of the recovery)
    double jrec_ratio = 1e1;       // JREC_RATIO: largest spread of the surviving row norms of R that recovers (wants_jrec)
    int jrec_min = 256;            // JREC_MIN: fewest surviving rows that recover
    bool lq_force_redo = false;    // LQ_FORCE_REDO: test hook, every list with an LQ block falls back to the plain iteration
    bool jrec_force_redo = false;  // JREC_FORCE_REDO: the same, only where rotations were recovered
    bool trace_redo = false;       // TRACE_REDO: one line per block with its route on stderr
    bool noqr = false;             // NOQR: no block enters the pipeline (direct iteration on the rows of A)
    bool nosmall = false;          // NOSMALL: no block goes to the in-LDS kernels (SVD and eigh)
    bool nomerge = false;          // NOMERGE: only blocks with min(m, n) >= 48 enter the pipeline (the split before the merge)
};

// recovered rotations: max |J' J'^T - 1| above this sends the list to the plain iteration with accumulation.  The
// recovered factor ends up, through orthogonal transformations only, in the U (or Vh) the caller checks to 1e-10; the
// iteration adds its own drift of 2e-12, so 2e-11 leaves a factor 4 to the tolerance (tests/test_svd_jrecover_model.py
// shows which blocks stay a further factor 10 inside it).
constexpr double JREC_BOUND = 2e-11;

// ---- workspace layout -------------------------------------------------------------------------------------------------------
struct SvdAux {           // what blocked_qr.h decides for one block (L = max(m, n), k = min(m, n), kp = svd_kp(k))
    size_t qr1;           // bqr_aux_bytes(L, k, L, k): the factorisation of A (or A^T)
    size_t complete;      // bqr_aux_bytes(k, k, k, k): the factorisation behind the completion of a block without LQ step
    size_t lq;            // bqr_aux_bytes(k, k, kp, k): the LQ factorisation
    size_t stop_doubles;  // panel steps x bqr_strip_slots(L): squared strip norms of the early stop of the first QR
};
struct SvdBlockLay {      // byte offsets into the workspace
    int m, n, k, L, kp;   // k = min, L = max, kp = k padded to 64
    bool tall;            // m >= n
    size_t sig;           // kp doubles: row norms            } the host-read header: one device-to-host copy
    size_t bad, dev;      // one double each: LQ flag, max |J' J'^T - 1|  }
    size_t ctl;           // two doubles: control words of the early stop }
    size_t Ac, aux, stop, W, J, rank, inv, nnull, Cq, Fc, aux2, Cn, Wc, Jc, Wq, aux3, Cq2, sig2, sigo;
    size_t idx;           // k int32: row-index list
};
struct SvdRegion {        // one carved piece, for whoever wants to walk them (tests/svd_plan.cpp)
    size_t off, bytes;
    int block;            // -1: shared
    const char* name;
};
// Contracts (checked in tests/svd_plan.cpp):
//  * [head_begin, head_begin + head_bytes) holds the sig arrays of all blocks, then bad[nmat], dev[nmat], ctl[2 nmat], and
//    nothing else: it rides in ONE device-to-host copy after the row norms.
//  * bad and dev are adjacent arrays of nmat doubles: flags_begin() .. + flags_bytes() is the copy of the redo decision.
//  * the index lists are contiguous in block order, k entries each, from idx_begin: one device copy rewrites all of them.
//  * every other piece starts on a multiple of 256 and the pieces are disjoint.
struct SvdLayout {
    std::vector<SvdBlockLay> blk;
    std::vector<SvdRegion> regions;
    size_t head_begin = 0, head_bytes = 0;
    size_t idx_begin = 0, idx_bytes = 0;
    size_t total = 0;
    size_t nmat() const { return blk.size(); }
    size_t flags_begin() const { return blk[0].bad; }
    size_t flags_bytes() const { return 2 * sizeof(double) * nmat(); }
    // index of a header word in the host copy of the header (doubles)
    size_t head_index(size_t off) const { return (off - head_begin) / sizeof(double); }
};
inline int svd_kp(int k) { return (k + 63) / 64 * 64; }
inline SvdLayout svd_layout(const std::vector<int>& m, const std::vector<int>& n, const std::vector<SvdAux>& aux)
{
    SvdLayout lay;
    const size_t nmat = m.size();
    lay.blk.resize(nmat);
    size_t off = 0;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    auto put = [&](size_t bytes, int block, const char* name) { // unaligned: the header words and the index lists
        const size_t o = off;
        lay.regions.push_back(SvdRegion{o, bytes, block, name});
        off += bytes;
        return o;
    };
    lay.head_begin = off;
    for (size_t b = 0; b < nmat; ++b) {
        SvdBlockLay& l = lay.blk[b];
        l.m = m[b];
        l.n = n[b];
        l.k = std::min(l.m, l.n);
        l.L = std::max(l.m, l.n);
        l.kp = svd_kp(l.k);
        l.tall = l.m >= l.n;
        l.sig = put(sizeof(double) * (size_t)l.kp, (int)b, "sig");
    }
    for (size_t b = 0; b < nmat; ++b) lay.blk[b].bad = put(sizeof(double), (int)b, "bad");
    for (size_t b = 0; b < nmat; ++b) lay.blk[b].dev = put(sizeof(double), (int)b, "dev");
    for (size_t b = 0; b < nmat; ++b) lay.blk[b].ctl = put(2 * sizeof(double), (int)b, "ctl");
    lay.head_bytes = off - lay.head_begin;
    off = al(off);
    for (size_t b = 0; b < nmat; ++b) {
        SvdBlockLay& l = lay.blk[b];
        auto take = [&](size_t bytes, const char* name) {
            const size_t o = put(bytes, (int)b, name);
            off = o + al(bytes);
            return o;
        };
        const size_t L = (size_t)l.L, k = (size_t)l.k, kp = (size_t)l.kp;
        l.Ac = take(sizeof(double) * L * k, "Ac");
        l.aux = take(aux[b].qr1, "aux");
        l.stop = take(sizeof(double) * std::max<size_t>(1, aux[b].stop_doubles), "stop");
        l.W = take(sizeof(double) * kp * kp, "W");
        l.J = take(sizeof(double) * kp * kp, "J");
        l.rank = take(sizeof(int32_t) * kp, "rank");
        l.inv = take(sizeof(int32_t) * kp, "inv");
        l.nnull = take(sizeof(int32_t), "nnull");
        l.Cq = take(sizeof(double) * L * k, "Cq");
        l.Fc = take(sizeof(double) * k * k, "Fc");
        l.aux2 = take(aux[b].complete, "aux2");
        l.Cn = take(sizeof(double) * k * k, "Cn");
        l.Wc = take(sizeof(double) * kp * kp, "Wc");
        l.Jc = take(sizeof(double) * kp * kp, "Jc");
        l.Wq = take(sizeof(double) * kp * kp, "Wq");
        l.aux3 = take(aux[b].lq, "aux3");
        l.Cq2 = take(sizeof(double) * k * k, "Cq2");
        l.sig2 = take(sizeof(double) * kp, "sig2");
        l.sigo = take(sizeof(double) * kp, "sigo");
    }
    lay.idx_begin = off;
    for (size_t b = 0; b < nmat; ++b) lay.blk[b].idx = put(sizeof(int32_t) * (size_t)lay.blk[b].k, (int)b, "idx");
    lay.idx_bytes = off - lay.idx_begin;
    lay.total = al(off);
    return lay;
}

// ---- deflation split --------------------------------------------------------------------------------------------------------
// numerical-rank threshold (numpy.linalg.matrix_rank's): ||A||_F * max(m, n) * eps, squared; ||A||_F = ||R||_F comes from
// the k row norms of R
inline double svd_rank_thr2(const double* sg, int k, int L)
{
    double fro2 = 0.0;
    for (int j = 0; j < k; ++j) fro2 += sg[j] * sg[j];
    const double sc = (double)L * kEps;
    return fro2 * sc * sc;
}
struct SvdSplit {
    std::vector<int32_t> good, nul; // ascending row indices
};
// Row j is kept when sg[j]^2 > thr2 (strictly).  cplx: rows 2a and 2a + 1 of an embedded complex block live or die together,
// by the larger of the two norms.  Up front thr2 is svd_rank_thr2; after the sweeps it is 0 -- a row norm is the square root
// of a double or zero, so its square is positive exactly when it is.
inline SvdSplit svd_split_rows(const double* sg, int k, double thr2, bool cplx)
{
    SvdSplit s;
    for (int j = 0; j < k; ++j) {
        const double v = cplx ? std::max(sg[j & ~1], sg[std::min(j | 1, k - 1)]) : sg[j];
        (v * v > thr2 ? s.good : s.nul).push_back(j);
    }
    return s;
}

// ---- route rules ------------------------------------------------------------------------------------------------------------
struct SvdSpread {
    double lo = 1e300, hi = 0.0;
    void add(double v)
    {
        lo = std::min(lo, v);
        hi = std::max(hi, v);
    }
};
// Second preconditioning step (LQ): the surviving rows R_g (r0 x k) are factored once more, R_g^T = Q2 R2, and the iteration
// runs on the rows of the r0 x r0 triangle R2 instead of the rows of R_g.  R2 R2^T is much closer to diagonal than R_g R_g^T
// (Drmac & Veselic, SIAM J. Matrix Anal. Appl. 29 (2008), sec. 3: the second QR is what makes one-sided Jacobi converge in a
// few sweeps): a theta of a DMRG bond (graded spectrum over 14 decades) needs 8 sweeps instead of 15, and the rows the rounds
// stream are r0 long instead of k.  With R2 = J'^T S Z^T (iteration: W' = S Z^T, rotations J')
//     R_g = Z S (Q2 [J'^T; 0])^T,
// so the pair the read-off expects is  W_equiv = S (Q2 [J'^T; 0])^T  and  J_equiv = Z^T, and the trailing k - r0 columns of
// Q2 are an orthonormal basis of the complement of R_g's row space: the completion of the up-front deflated rows needs no QR
// of its own any more.
// Not for every block.  A FULL-RANK, well-conditioned large block (row norms of R within 1e4 of each other, k >= 128)
// converges in the same number of sweeps on R itself -- 9-11 against 9-10 -- so the second factorisation (k / 32 panel steps
// of ~170 us) is never repaid now that a sweep is cheap: Gaussian 1024^2 26.6 -> 22.9 ms, four 512^2 11.3 -> 9.9 ms
// (scripts/lq_choice_probe.py).  Rank-deficient blocks keep it (the iteration shrinks to r0 x r0 and the completion falls out
// of Q2), graded ones too (fewer sweeps and the better accuracy of the small values), small ones too (a sweep costs a launch
// there).  CYB_SVD_LQ_ALWAYS=1: every block.
// lo, hi: spread of ALL k row norms of R.
inline bool wants_lq(int r0, int k, double lo, double hi, const SvdSwitches& sw)
{
    const bool skip = !sw.lq_always && r0 == k && k >= sw.lq_skip_k && hi <= sw.lq_skip_ratio * lo;
    return !sw.nolq && r0 >= 2 && !skip;
}
// Rotation recovery: which LQ blocks iterate WITHOUT accumulating J' (it is rebuilt from S Z^T and R2 after the sweeps, see
// SvdPipeline::stage_iteration).  The rebuilt factor carries the relative error the iteration leaves in a row of S Z^T
// (eps sqrt(32 rounds sweeps), 3e-14 at r0 = 1024) times up to the condition of R2, which the spread of the surviving row
// norms of R -- already on the host -- follows within a factor 10.  tests/test_svd_jrecover_model.py: the default ratio is
// the largest power of ten that keeps every admitted family 10x inside JREC_BOUND and refuses the others with that factor 10
// to spare; it admits the blocks of a theta = A.B (condition ~10) and refuses a full-rank Gaussian block (4e3) and every
// graded spectrum.
// Below CYB_SVD_JREC_MIN rows the accumulation costs nothing and the recovery three launches (chi = 1024 step, blocks of
// r0 = 180 .. 212: 4.85 ms without, 5.0 - 5.5 with; neutral from 256).  Embedded complex blocks are excluded: the recovery
// product does not keep the pair structure bit for bit.
// lo, hi: spread of the row norms of R over the r0 SURVIVING rows.
inline bool wants_jrec(bool lq, int r0, double lo, double hi, bool cplx, const SvdSwitches& sw)
{
    if (!lq || sw.nojrec || cplx || r0 < sw.jrec_min) return false;
    return hi <= sw.jrec_ratio * lo;
}

// ---- null-row columns -------------------------------------------------------------------------------------------------------
// Every null row of an LQ block has its unit vector in Cq2 = Q2 [J'^T 0; 0 I] already: a row deflated up front takes the next
// of the trailing columns r0 + t (the complement of R_g's row space), a row the read-off of the LQ iteration found
// numerically null (sigma_i^2 <= thr2) its own compact column -- its position in good0.  good0 and nul are ascending.
inline std::vector<int32_t> svd_null_columns(const std::vector<int32_t>& good0, const int32_t* nul, int n_nul)
{
    std::vector<int32_t> cols;
    const int r0 = (int)good0.size();
    int t = 0;
    size_t g = 0;
    for (int q = 0; q < n_nul; ++q) {
        const int32_t j = nul[q];
        while (g < good0.size() && good0[g] < j) ++g;
        if (g < good0.size() && good0[g] == j) cols.push_back((int32_t)g);
        else cols.push_back((int32_t)(r0 + t++));
    }
    return cols;
}

// ---- compact positions ------------------------------------------------------------------------------------------------------
// Compact row of every full-size row (-1: deflated up front), k entries per matrix behind each other: the J side is read off
// the compact rotations without a scatter into the full-size J (j_to_cq_kernel).  Appends block b and returns its offset.
inline int64_t svd_append_positions(std::vector<int32_t>& pos_all, int k, const std::vector<int32_t>& good0)
{
    const size_t o = pos_all.size();
    pos_all.resize(o + (size_t)k, -1);
    for (size_t g = 0; g < good0.size(); ++g) pos_all[o + (size_t)good0[g]] = (int32_t)g;
    return (int64_t)o;
}

// ---- list split -------------------------------------------------------------------------------------------------------------
enum class SvdRoute { tiny, direct, pipeline };
struct SvdShape {
    int64_t m, n;
    bool fits; // svd_small_fits(m, n): min <= 64, max <= 128, the whole iteration in LDS with one workgroup per block
};
// tiny: the in-LDS kernel (svd_small.hip) -- when the fitting blocks are the whole list or many (16): a few tiny sectors next
// to large ones (the two or three smallest blocks of a chi=4096 theta) ride along in the rounds of the large blocks for free,
// whereas the fused kernel would sit in front of the pipeline on the same stream (0.66 ms of a 53 ms call).  Never for
// embedded complex blocks: one pipeline for every size.
// pipeline: every other block with min(m, n) >= 2, whatever its size.  The smaller blocks of a list join the large ones
// (their panels and sweeps ride along in the same launches) instead of forming a second, serial iteration behind them -- a
// DMRG bond at chi = 256 has sectors from 4 x 4 to 140 x 140 in one call -- and the direct iteration (run_jacobi on the rows
// of A) has no deflation of numerically zero rows: a rank-deficient 38 x 135 block with 105 zero columns kept rotating
// rounding noise for 40 sweeps (scripts/tensor_fuzz.py, seed 11; the up-front deflation of the pipeline takes those rows out
// before the first sweep).  CYB_SVD_NOMERGE keeps the old split (min(m, n) >= 48) for the tests; embedded blocks enter from 1.
// direct: the rest (vectors; everything with CYB_SVD_NOQR).
inline std::vector<SvdRoute> svd_split_list(const std::vector<SvdShape>& blocks, bool embedded, const SvdSwitches& sw)
{
    size_t n_fit = 0;
    for (const SvdShape& d : blocks) n_fit += d.fits ? 1 : 0;
    const bool use_small = !embedded && !sw.nosmall && (n_fit == blocks.size() || n_fit >= 16);
    const int64_t large_min = embedded ? 1 : sw.nomerge ? 48 : 2;
    std::vector<SvdRoute> route;
    for (const SvdShape& d : blocks)
        route.push_back(use_small && d.fits ? SvdRoute::tiny
                        : !sw.noqr && std::min(d.m, d.n) >= large_min ? SvdRoute::pipeline
                                                                      : SvdRoute::direct);
    return route;
}

} // namespace cyb
