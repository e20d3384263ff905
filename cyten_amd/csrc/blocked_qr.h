// Batched blocked Householder QR on column-major working matrices (internal).
//
//   A = Q R,  Q = H_0 H_1 ... H_{k-1},  H_j = I - tau_j v_j v_j^T  (LAPACK dgeqrf conventions),
//   panels of NBK columns: unblocked Householder inside the panel (one workgroup per matrix),
//   compact-WY block reflector  I - V T V^T  applied to the trailing matrix / to Q's columns in
//   32-column strips, one launch per panel step for the WHOLE batch (two when the strips' rows are split).
#pragma once
#include "common.h"

namespace cyb {

constexpr int NBK = 32;

struct BqrMat {
    double* Ac;      // col-major m x n (element (i,c) at Ac[c*ld + i]); overwritten: R in the upper triangle
    int64_t ld;      // >= m
    int32_t m, n, k; // k = min(m,n)
    double* V;       // col-major m x k (same ld): explicit unit-lower-trapezoidal reflectors
    double* T;       // ceil(k/NBK) blocks of NBK x NBK (row-major, upper triangular)
    double* tau;     // k
    double* scratch; // scr_total doubles: the wide application of Q (bqr_apply_q) keeps the row-chunk partials of a whole
                     // group's W1 here; the strips need none of it (still sized for at least (1 + kWSplit) * scr_half)
    int64_t scr_half; // NBK * max(n, kc_max)
    int64_t scr_total = 0; // doubles behind `scratch` (set by bqr_carve)
    int32_t v_zeroed = 0; // the caller has zero-filled V (a memset of its workspace): the panel kernels skip the rows above a panel
    // Early stop (SVD preconditioner only): ctl -> 2 zeroed doubles, parts -> ceil(n / NBK) * bqr_strip_slots(m) doubles, stop_rel2 > 0: the
    // factorisation stops once ||A[j:, j:]||_F^2 <= stop_rel2 x (largest trailing norm seen); the remaining reflectors are the
    // identity (T = 0: the caller's workspace must be zeroed), the remaining rows of R are that trailing block's upper
    // triangle, at the rounding level of the matrix.
    double* ctl = nullptr;
    double* parts = nullptr;
    double stop_rel2 = 0.0;
    int32_t reflect_always = 0; // a column whose tail below the pivot is exactly zero is still reflected (H = I - 2 e e^T,
                                // R_jj = -alpha) instead of LAPACK's tau = 0: the diagonal of R then ALWAYS has the sign
                                // -sign(alpha), which keeps the R of an interleaved complex embedding structured (the
                                // last column of a square matrix, whose partner column was reflected)
};

// bytes of V + T + tau + scratch for an m x n matrix whose Q will be applied to at most kc columns
size_t bqr_aux_bytes(int64_t m, int64_t n, int64_t ld, int64_t kc);
// carve V/T/tau/scratch out of `base` (256-B aligned pieces); returns bytes used
size_t bqr_carve(BqrMat& q, char* base, int64_t kc);

// number of row chunks (workgroups) a strip of `rows` rows is split into by the two-launch form of the block-reflector
// application; a factorisation with early stop needs ceil(n / NBK) * bqr_strip_slots(m) doubles of `parts`
int bqr_strip_slots(int64_t rows);

// factor every matrix (asynchronous on ctx->stream)
int bqr_factor(cyb_ctx_t ctx, const std::vector<BqrMat>& mats);

struct BqrTarget {
    int32_t mat;  // index into mats
    double* C;    // col-major m x kc, ld = ldc
    int64_t ldc;
    int32_t kc;
    int32_t n_pan = -1; // panels the factorisation did not skip (a matrix with early stop: ctl[0] - 1 once ctl[0] != 0, read by
                        // the caller); -1: all.  The wide route stages no group behind it and needs it for a matrix with ctl.
};
// C <- Q C for every target (asynchronous). At most one target per matrix per call (the targets
// share the matrix' scratch), kc <= the kc the matrix was carved for.
// Two routes: 32-column strips, panel by panel, or groups of CYB_QR_APPLY_WIDTH reflector columns through the grouped GEMM
// (merged T factors, two GEMM launches per group).  A target qualifies for the wide route by its shape (wide_target); the
// qualifying targets of ONE application take it only if their columns sum to kWideMinCols, otherwise the whole application
// stays on strips (split_routes).  CYB_QR_TRACE_ROUTE: one line on stderr per application with the outcome.
int bqr_apply_q(cyb_ctx_t ctx, const std::vector<BqrMat>& mats, const std::vector<BqrTarget>& targets);
// Two applications that do not depend on each other in one call: targets[0 : n_first] and targets[n_first :] are each
// routed exactly as a call of their own would route them (the shape rule sums the columns of ONE application), the strip
// targets of each run as that call would run them, and the wide targets of both share their launches (one prelude,
// every group launch carries both chains).  The rule above holds for the whole list: one target per matrix.
int bqr_apply_q_pair(cyb_ctx_t ctx, const std::vector<BqrMat>& mats, const std::vector<BqrTarget>& targets, size_t n_first);

// Batched tile transpose  out[r*ldo + c] = in[c*ldi + r]  for r < R, c < C  (row-major <-> col-major).
// upper != 0: entries with r > c or r >= rlim are written as 0 (extraction of R).
// plain != 0: no transpose, out[r*ldo + c] = in[r*ldi + c] (2-D copy with different leading dimensions).
// idx != null: a permutation on the READ side, of the strided index of `in` -- out[r*ldo + c] = in[idx[c]*ldi + r], or
// with plain out[r*ldo + c] = in[idx[r]*ldi + c]: the reads stay contiguous runs and the writes coalesced.
struct XposeDesc {
    const double* in;
    double* out;
    int64_t ldi, ldo;
    int32_t R, C, upper, rlim;
    int32_t plain, pad;
    const int32_t* idx = nullptr;
};
int xpose_batched(cyb_ctx_t ctx, const std::vector<XposeDesc>& descs);
// C (col-major m x kc, ld) = first kc columns of the identity
struct EyeDesc {
    double* C;
    int64_t ld;
    int32_t m, kc;
    int32_t col0, pad; // column c of C is the unit vector e_{c + col0}
};
int eye_cols_batched(cyb_ctx_t ctx, const std::vector<EyeDesc>& descs);

} // namespace cyb
