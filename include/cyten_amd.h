/*
 * cyten_amd.h -- C-ABI of the MI355X-native block backend for cyten.
 *
 * This is the drop-in boundary: everything cyten's `BlockBackend`
 * (reference: include/cyten/block_backend/block_backend.h:18-500) needs from a
 * device is reachable through the plain-C entry points below.  No torch, no
 * pybind, no C++ types cross this boundary: device pointers are `void*` /
 * `double*` obtained from any HIP allocator (hipMalloc, a torch tensor's
 * data_ptr, ...), sizes are int64_t, and every call returns an int status
 * (0 = ok) with a thread-local message retrievable via cyb_last_error().
 *
 * Design notes:
 *  - The reference API is one-block-at-a-time (matrix_dot / matrix_svd / ...,
 *    block_backend.h:436-472).  The hardware wants whole block lists, so every
 *    hot entry point here is *grouped*: one call = all blocks of one tensor op,
 *    one (or a few) kernel launches.  The single-block reference calls are the
 *    n=1 special case.
 *  - All work is enqueued on the context's HIP stream and is asynchronous with
 *    respect to the host unless stated otherwise.
 *  - fp64 is the arithmetic type of the hot path (BASELINE.json).  Data
 *    movement entry points are byte-size generic (elem_size 1, 4, 8, 16).
 *  - DTYPE RESTRICTION (deliberate).  The reference's Dtype set is bool, int64,
 *    float32, complex64, float64, complex128 (include/cyten/block_backend/
 *    dtypes.h:12-21).  Arithmetic entry points exist for float64 (`_f64`) and
 *    complex128 (`_c128`: interleaved (re, im) storage, numpy's layout); bool
 *    is a 1-byte storage type for masks and comparison results
 *    (cyb_compare_f64, cyb_count_nonzero_u8, cyb_convert_u8_f64).  float32,
 *    complex64 and int64 blocks have NO arithmetic here: they can be moved
 *    (cyb_copy_strided_batched with elem_size 4 / 8) but the host mirror
 *    (HipBlockBackend.to_dtype) refuses them, and the Array-API namespace of
 *    integration/ keeps such data -- index arrays from argsort / argmin, int64
 *    scalars -- on the host.  Nothing on the tdot / SVD / QR / eigh path of
 *    cyten uses them.
 *  - A change of the context's stream (cyb_ctx_set_stream) orders the new
 *    stream behind everything enqueued on the old one (the workspaces and the
 *    descriptor ring are shared).
 */
#ifndef CYTEN_AMD_H
#define CYTEN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CYB_VERSION 100 /* 0.1.0 */

/* status codes */
enum {
    CYB_OK = 0,
    CYB_ERR_INVALID = 1,  /* bad argument (-> std::invalid_argument / ValueError in the adapter) */
    CYB_ERR_HIP = 2,      /* a HIP runtime call failed */
    CYB_ERR_NOCONV = 3,   /* an iterative decomposition did not converge (-> LinAlgError) */
    CYB_ERR_NOMEM = 4,
    CYB_ERR_UNSUPPORTED = 5
};

typedef struct cyb_ctx_s* cyb_ctx_t;

/* ---- context / stream / errors ------------------------------------------------------------ */

/* Version of the library (CYB_VERSION it was built with). */
int cyb_version(void);
/* Thread-local message of the last failing call ("" if none). */
const char* cyb_last_error(void);
/* Create a context on HIP device `device`. `stream` is a hipStream_t (may be NULL = the
 * device's null stream); the context does not own it.
 * Mirrors the per-device backend singleton of the reference
 * (src/block_backend/torch.cpp:669-695, numpy.cpp:411-432). */
int cyb_ctx_create(cyb_ctx_t* out, int device, void* stream);
int cyb_ctx_destroy(cyb_ctx_t ctx);
int cyb_ctx_set_stream(cyb_ctx_t ctx, void* stream);
/* Block the host until everything enqueued on the context's stream is done.
 * Replaces BlockBackend::synchronize (block_backend.h:478-479). */
int cyb_ctx_sync(cyb_ctx_t ctx);
/* Device properties the host planner needs. */
int cyb_device_info(cyb_ctx_t ctx, int* n_cu, int* lds_bytes, int64_t* hbm_bytes, char* arch, int arch_len);

/* ---- raw memory (used by hosts that do not bring their own allocator) ---------------------- */
int cyb_malloc(cyb_ctx_t ctx, void** out, size_t bytes);
int cyb_free(cyb_ctx_t ctx, void* ptr);
int cyb_memcpy_h2d(cyb_ctx_t ctx, void* dst, const void* src, size_t bytes); /* async on stream */
int cyb_memcpy_d2h(cyb_ctx_t ctx, void* dst, const void* src, size_t bytes); /* synchronous */
int cyb_memcpy_d2d(cyb_ctx_t ctx, void* dst, const void* src, size_t bytes); /* async */
int cyb_memset(cyb_ctx_t ctx, void* dst, int byte, size_t bytes);            /* async */

/* ---- timing (HIP events on the context's stream) ------------------------------------------- */
typedef struct cyb_event_s* cyb_event_t;
int cyb_event_create(cyb_event_t* out);
int cyb_event_destroy(cyb_event_t ev);
int cyb_event_record(cyb_ctx_t ctx, cyb_event_t ev);
int cyb_event_elapsed_ms(cyb_event_t start, cyb_event_t stop, float* ms); /* syncs on stop */
/* Measurement hook: the NEXT asynchronous grouped-GEMM launch of this context (cyb_gemm_grouped_enqueue_f64,
 * cyb_compose_plan_enqueue_f64) records `start` / `stop` on the stream directly around its kernel(s), i.e. behind the
 * descriptor upload -- the kernel duration rocprofv3 reports, not the enqueue.  One shot; NULL events clear it. */
int cyb_ctx_time_next_gemm(cyb_ctx_t ctx, cyb_event_t start, cyb_event_t stop);

/* ---- grouped block GEMM (tdot hot loop) ------------------------------------------------------
 * Replaces the loop  block = bb.matrix_dot(a,b); block = block + bb.matrix_dot(a',b'); ...
 * of abelian_compose_worker (reference src/backends/abelian.cpp:1424-1460), one
 * NumpyBlockBackend::matrix_dot = np.dot per pair (src/block_backend/numpy.cpp:1218-1225),
 * and FusionTreeBackend::compose (src/backends/fusion_tree_backend.cpp:669-698).
 *
 * One *problem* is one result block  C (M x N, row stride ldc, unit column stride)
 *      C = alpha * sum_{s in segments} A_s(M x K_s) * B_s(K_s x N)  + beta * C
 * The segments are the K-split pairs the reference accumulates with Block::operator+; here
 * they are accumulated in registers inside one tile pass (no extra C traffic).
 * Operands are strided *views*: element (i,k) of A_s is A[i*a_rs + k*a_cs]; one of the two
 * strides must be 1 (row- or column-major view, i.e. permuted/transposed blocks need no copy).
 */
typedef struct {
    const double* A;
    const double* B;
    int64_t K;
    int64_t a_rs, a_cs; /* element strides of A: rows (M index), cols (K index) */
    int64_t b_rs, b_cs; /* element strides of B: rows (K index), cols (N index) */
} cyb_gemm_seg;

typedef struct {
    double* C;
    int64_t M, N;
    int64_t ldc;       /* row stride of C in elements (>= N) */
    int32_t seg_begin; /* segments [seg_begin, seg_end) of the seg array belong to this problem */
    int32_t seg_end;
    double alpha, beta; /* beta == 0: C is not read */
} cyb_gemm_prob;

typedef struct cyb_gemm_plan_s* cyb_gemm_plan_t;

/* Build a launch plan (tile queue + device-resident descriptors) for a block list. Host arrays
 * are copied; pointers inside them must stay valid device pointers while the plan is run. */
int cyb_gemm_plan_create(cyb_ctx_t ctx, cyb_gemm_plan_t* out,
                         const cyb_gemm_prob* probs, int64_t n_probs,
                         const cyb_gemm_seg* segs, int64_t n_segs);
int cyb_gemm_plan_run(cyb_ctx_t ctx, cyb_gemm_plan_t plan);
int cyb_gemm_plan_destroy(cyb_gemm_plan_t plan);
/* algorithmic flops (sum 2*M*N*K) and bytes (8*(MK+KN+MN)) of the plan, number of launches/tiles */
int cyb_gemm_plan_info(cyb_gemm_plan_t plan, double* flops, double* bytes, int64_t* n_tiles, int32_t* n_launches);
/* convenience: create + run + destroy (synchronises the device) */
int cyb_gemm_grouped_f64(cyb_ctx_t ctx,
                         const cyb_gemm_prob* probs, int64_t n_probs,
                         const cyb_gemm_seg* segs, int64_t n_segs);
/* One-shot asynchronous form: validates, stages the descriptors through the context's pinned upload
 * ring and enqueues the launch on the context's stream -- no plan object, no device allocation, no
 * host synchronisation.  This is what a block list that is contracted once (every compose of a Krylov
 * matvec, abelian.cpp:1424-1460) should use; the operands must stay alive until the stream reaches
 * the launch (stream-ordered allocators give that for free). */
int cyb_gemm_grouped_enqueue_f64(cyb_ctx_t ctx,
                                 const cyb_gemm_prob* probs, int64_t n_probs,
                                 const cyb_gemm_seg* segs, int64_t n_segs);
/* Back-to-back v_mfma_f64_16x16x4_f64 issue micro-benchmark: returns measured TFLOP/s of the
 * chip (every CU issuing, `iters` MFMAs per wave on independent accumulators held in AGPRs;
 * waves_per_simd = accumulators * 100 + waves, accumulators 1/2/4/8, default 4).  The measured fp64
 * MFMA ceiling next to the spec one: 74.8 of 78.6 TFLOP/s on MI355X. */
int cyb_mfma_f64_peak(cyb_ctx_t ctx, int iters, int waves_per_simd, double* tflops, double* ms);

/* ---- batched per-block decompositions ----------------------------------------------------------
 * One descriptor per sector block; the whole block list of a tensor goes in one call.
 * All matrices are row-major (C order, as numpy blocks are) with explicit row strides.
 */

/* Thin SVD  A(m x n) = U(m x k) diag(S(k)) Vh(k x n),  k = min(m,n),  S descending, >= 0.
 * Replaces NumpyBlockBackend::matrix_svd = scipy.linalg.svd(a, full_matrices=False)
 * (src/block_backend/numpy.cpp:1247-1297), called per block from AbelianBackend::svd
 * (src/backends/abelian.cpp:3517-3518) and FusionTreeBackend::svd (fusion_tree_backend.cpp:2211).
 * A is not modified.
 * Leading dimensions (every entry and every route): lda >= n, ldu >= k, ldvh >= n for a block with both extents positive,
 * else the call is CYB_ERR_INVALID and nothing is read, uploaded or launched.  Nothing outside the addressed elements is
 * written: the gaps of a strided U / Vh and everything around S stay as they were. */
typedef struct {
    const double* A; int64_t lda;
    int64_t m, n;
    double* U; int64_t ldu;   /* m x k */
    double* S;                /* k */
    double* Vh; int64_t ldvh; /* k x n */
} cyb_svd_desc;
/* info[i] (host array, may be NULL): number of Jacobi sweeps used for block i, or <0 if it did
 * not converge within max_sweeps (then the call returns CYB_ERR_NOCONV).  The call synchronises
 * the stream when info != NULL. */
int cyb_svd_batched_f64(cyb_ctx_t ctx, const cyb_svd_desc* descs, int64_t n, int32_t* info);

/* The same with options, for the caller that TRUNCATES afterwards (truncated_svd_py, /root/reference/src/tensors/
 * decompositions.cpp:673-712: svd -> truncate_singular_values -> svd_apply_mask discards every vector that is not kept).
 *   flags & CYB_SVD_SKIP_NULL_VECTORS: singular vectors of numerically zero singular values (sigma below
 *       |A|_F max(m,n) eps, numpy.linalg.matrix_rank's threshold) are not completed to an orthonormal set: the
 *       corresponding columns of U / rows of Vh are unspecified (zero on the normalised side).  S and all other vectors
 *       are exactly those of cyb_svd_batched_f64.  Saves the second blocked QR of every rank-deficient block -- every
 *       block of a two-site theta = A.B is rank-deficient by construction.
 *   rank[i] (host array, may be NULL): number of singular values of block i above that threshold; a caller that keeps
 *       more than rank[i] values of a block must call cyb_svd_batched_f64 for it instead. */
#define CYB_SVD_SKIP_NULL_VECTORS 1
/* every block is the interleaved real embedding M(A) of a complex block: entry a + ib -> [[a, -b], [b, a]], 2m x 2n, both
 * extents even.  The factors come back embedded the same way (U: 2m x 2k, S: 2k with every value twice, Vh: 2k x 2n): real
 * column 2a of U IS complex column a (rows 0::2 real parts, rows 1::2 imaginary parts), real row 2a of Vh IS complex row a
 * (columns 0::2 real parts, columns 1::2 minus the imaginary parts), and the two belong to the same singular triplet.  Where
 * the block is rank deficient or graded over many decades the real factors are orthogonal but structured only up to
 * eps * sigma_max / sigma_j: a caller that needs complex orthonormality there re-orthonormalises those columns
 * (cyten_amd/block_backend.py, _complex_svd_embedded).  CYB_ERR_UNSUPPORTED: the list has too many rows for one persistent
 * sweep launch (use cyb_svd_batched_c128).  numpy.cpp:1247-1297 for complex128 blocks, on the float64 block engine
 * (DESIGN.md section 4.5b). */
#define CYB_SVD_EMBEDDED_COMPLEX 2
int cyb_svd_batched_ex_f64(cyb_ctx_t ctx, const cyb_svd_desc* descs, int64_t n, int32_t* info, int32_t flags, int32_t* rank);

/* QR  A(m x n) = Q R.  economic: Q m x k, R k x n (k=min(m,n)); full: Q m x m, R m x n.
 * Replaces NumpyBlockBackend::matrix_qr = scipy.linalg.qr(a, mode=...) (numpy.cpp:1236-1245);
 * matrix_lq (block_backend.cpp:1033-1040) is built on it by the host.
 * Sign convention as LAPACK dgeqrf (R diagonal may be negative).
 * Leading dimensions: lda >= n, ldq >= k (full: m), ldr >= n for a block with both extents positive, else the call is
 * CYB_ERR_INVALID and no output is written.  R is written whole (zeros below the diagonal and in rows k .. m-1 of a full
 * R); the gaps of a strided Q / R stay as they were. */
typedef struct {
    const double* A; int64_t lda;
    int64_t m, n;
    double* Q; int64_t ldq;
    double* R; int64_t ldr;
    int32_t full;
} cyb_qr_desc;
int cyb_qr_batched_f64(cyb_ctx_t ctx, const cyb_qr_desc* descs, int64_t n);

/* Hermitian (real symmetric) eigendecomposition  A(n x n) = V diag(W) V^T,  W ascending.
 * Replaces NumpyBlockBackend::eigh = np.linalg.eigh (numpy.cpp:658-680). Only the lower
 * triangle convention of LAPACK is not relied upon: A is assumed symmetric.
 * V may be NULL (eigvalsh, numpy.cpp:682-698); ldv is not looked at then.
 * Leading dimensions (every entry and every route): lda >= n, and ldv >= n where V != NULL, for a block with n > 0, else
 * the call is CYB_ERR_INVALID and nothing is read, uploaded or launched.  The gaps of a strided V stay as they were. */
typedef struct {
    const double* A; int64_t lda;
    int64_t n;
    double* W;
    double* V; int64_t ldv;
} cyb_eigh_desc;
int cyb_eigh_batched_f64(cyb_ctx_t ctx, const cyb_eigh_desc* descs, int64_t n, int32_t* info);
/* flags & CYB_EIGH_EMBEDDED_COMPLEX: every block is the interleaved real embedding M(H) (2n x 2n, n even in the embedding's
 * extents) of a complex Hermitian block: W comes back with every eigenvalue twice (2n values), real column 2a of V is the
 * complex eigenvector a (rows 0::2 real parts, rows 1::2 imaginary parts) -- exactly structured, no QR step is involved.
 * CYB_ERR_UNSUPPORTED as for the SVD.  np.linalg.eigh of complex128 blocks (numpy.cpp:658-680) on the float64 block engine. */
#define CYB_EIGH_EMBEDDED_COMPLEX 2
int cyb_eigh_batched_ex_f64(cyb_ctx_t ctx, const cyb_eigh_desc* descs, int64_t n, int32_t* info, int32_t flags);

/* ---- data movement: strided N-d copies (permute_axes / reshape-copy / get_item / set_item,
 *      combine_legs / split_legs sub-block scatter/gather) ------------------------------------
 * dst[sum_d i_d*dst_strides[d]] = src[sum_d i_d*src_strides[d]]  for i_d in [0, shape[d]).
 * Strides in elements of elem_size bytes (1, 4, 8 or 16; any other size is CYB_ERR_INVALID); dst and src are
 * aligned to elem_size.  A stride may be 0 (a broadcast read on the source side) or negative; a destination
 * whose strides make two index tuples meet at one address is the caller's error and is not checked.
 * ndim <= CYB_MAX_NDIM. Replaces the numpy
 * views of numpy.cpp:924-931 (permute_axes), :1057-1064 (reshape) once a contiguous result is
 * needed, and the `new_block[slices] = combined` scatter of abelian.cpp:1212-1214 /
 * `old_block[slices]` gather of abelian.cpp:3414-3427.  The whole list is one launch. */
#define CYB_MAX_NDIM 8
typedef struct {
    void* dst;
    const void* src;
    int32_t ndim;
    int32_t conj; /* 1: complex-conjugate while copying (elem_size 16 = complex128 only) */
    int64_t shape[CYB_MAX_NDIM];
    int64_t dst_strides[CYB_MAX_NDIM];
    int64_t src_strides[CYB_MAX_NDIM];
} cyb_copy_desc;
int cyb_copy_strided_batched(cyb_ctx_t ctx, const cyb_copy_desc* descs, int64_t n, int32_t elem_size);

/* ---- placement plans: the same strided copies for a block STRUCTURE that comes back (combine_legs / split_legs of the same
 *      legs and block table, bond after bond).  A record names its two blocks by their row in two address tables instead of
 *      by address:  dst_ptrs[dst_block][dst_offset + sum_d i_d*dst_strides[d]] = src_ptrs[src_block][src_offset + sum_d
 *      i_d*src_strides[d]], offsets and strides in elements of elem_size bytes (8 or 16).
 * create (synchronous, once per structure): validates (ndim <= CYB_MAX_NDIM, block numbers inside the tables, extents and
 *      offsets >= 0), merges axes, decides per record between the row-run and the LDS-tiled transposing kernel, cuts the
 *      work items and stores records and items in device memory the plan owns -- what cyb_copy_strided_batched does per call.
 * enqueue (asynchronous): src_ptrs[n_src], dst_ptrs[n_dst] = device addresses of the blocks at hand (host arrays, copied
 *      by ONE upload; an address may be 0 only for a block no non-empty record names); at most one launch per kernel class.
 *      reverse = 1 copies the other way, dst side -> src side (the gather of split_legs); the records of that direction
 *      are classified on its first use.  Nothing is checked per element: the caller vouches that every block holds what
 *      the records address.  Records may not overlap on the side that is written.
 * destroy: waits for the device, then frees the plan's memory. */
typedef struct {
    int32_t src_block, dst_block; /* rows of the two address tables given at enqueue */
    int32_t ndim, pad;
    int64_t src_offset, dst_offset;
    int64_t shape[CYB_MAX_NDIM];
    int64_t src_strides[CYB_MAX_NDIM];
    int64_t dst_strides[CYB_MAX_NDIM];
} cyb_place_rec;
typedef struct cyb_place_plan_s* cyb_place_plan_t;
int cyb_place_plan_create(cyb_ctx_t ctx, const cyb_place_rec* recs, int64_t n, int64_t n_src, int64_t n_dst, int32_t elem_size,
                          cyb_place_plan_t* out);
int cyb_place_plan_enqueue(cyb_ctx_t ctx, cyb_place_plan_t plan, const int64_t* src_ptrs, const int64_t* dst_ptrs, int32_t reverse);
int cyb_place_plan_destroy(cyb_place_plan_t plan);

/* ---- BLAS-1 class block-list ops (Lanczos / truncation callers: norm, inner,
 *      linear_combination, mul, scale_axis; numpy.cpp:898-913, :815-842, :1358-1385) ----------- */
typedef struct {
    const double* x; /* contiguous */
    const double* y; /* contiguous, may be NULL where unused */
    double* out;     /* contiguous, may alias x or y, may be NULL where unused */
    int64_t n;
} cyb_vec_desc;
/* result[0] = sum over all list entries of sum_i x_i*y_i  (y == NULL: x_i*x_i); device scalar */
int cyb_dot_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev);
/* per-entry results: result_dev[j] = sum_i x_i*y_i of entry j */
int cyb_dot_each_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev);
/* out = a*x + b*y  for every entry (y may be NULL with b ignored) */
int cyb_axpby_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double a, double b);
/* result_dev[0] = max_i |x_i| over the whole list; NaN if any element of any entry is NaN (np.max(np.abs(x))), 0 for an
 * empty list */
int cyb_maxabs_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev);
/* elementwise binary op on contiguous lists: out = x (op) y; op: 0 add, 1 sub, 2 mul, 3 div, 4 pow (Block::pow(Block), numpy.cpp power) */
int cyb_binary_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, int32_t op);
/* elementwise unary op: out = f(x) (out may be x); op: 0 abs, 1 sqrt, 2 exp, 3 log, 4 neg, 5 square, 6 reciprocal,
 * 7 round to float32 (the cast-on-store of float32 / complex64 blocks, dtypes.h:12-21: they are held in double words),
 * 8 truncate toward zero (int64 blocks) */
int cyb_unary_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, int32_t op);

/* elementwise unary op with one parameter: op 0 cutoff_inverse (|x| < param ? 0 : 1/x, numpy.cpp:645-656),
 * 1 stable_log (x > param ? log x : 0, numpy.cpp:1088-1098), 2 pow (x ** param, Block::pow numpy.cpp:265-270),
 * 3 angle of a real number (numpy.cpp:587-594; param ignored) */
int cyb_unary_param_batched_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, int32_t op, double param);
/* out[i] = x[i] (op) y[i]  (y == NULL: x[i] (op) scalar) as one byte per element, 0 / 1: the boolean blocks of
 * Block::operator< <= > >= == != (numpy.cpp:229-263); op: 0 lt, 1 le, 2 gt, 3 ge, 4 eq, 5 ne.  Contiguous. */
int cyb_compare_f64(cyb_ctx_t ctx, const double* x, const double* y, double scalar, uint8_t* out, int64_t n, int32_t op);
/* out[i] = x[i] ? 1.0 : 0.0  (to_dtype of a boolean block, numpy.cpp:1131-1138) */
int cyb_convert_u8_f64(cyb_ctx_t ctx, const uint8_t* x, double* out, int64_t n);
/* result_dev[0] = number of non-zero bytes: any / all / sum_all of a boolean block (numpy.cpp:568-575, 596-603) */
int cyb_count_nonzero_u8(cyb_ctx_t ctx, const uint8_t* x, int64_t n, uint64_t* result_dev);
/* extremum of a contiguous vector together with its flat index, ties resolved to the lowest index like np.argmax /
 * np.argmin: mode 0 max (numpy.cpp:871-878), 1 min (:889-896, argmin :552-566), 2 max |x| (abs_argmax :533-550).
 * result_dev[0] = the maximised key (x, -x or |x|), result_dev[1] = the index as an int64 bit pattern.
 * NaN rule (np.max / np.min / np.argmax / np.argmin): a NaN ranks above every number in every mode -- if the vector
 * holds one, the key is NaN and the index is that of the first NaN.  -0.0 and 0.0 compare equal (lowest index wins). */
int cyb_extremum_f64(cyb_ctx_t ctx, const double* x, int64_t n, int32_t mode, double* result_dev);
/* result_dev[0] = number of elements that FAIL np.isclose(x, y, rtol, atol): an element passes when x == y (equal
 * infinities included) or when both are finite and |x - y| <= atol + rtol * |y|.  NaN rule: a NaN on either side fails
 * (equal_nan=False).  is_complex: n interleaved (re, im) elements, |.| the modulus, finite = both parts finite.
 * np.allclose is `result == 0` (numpy.cpp:578-585).  Contiguous operands. */
int cyb_allclose_count(cyb_ctx_t ctx, const double* x, const double* y, int64_t n, int32_t is_complex, double rtol, double atol,
                       uint64_t* result_dev);

/* out[i, j, k] = x[i, j, k] * f[j]  for a block viewed as (outer, axis, inner), contiguous.
 * Replaces scale_axis (numpy.cpp:1373-1385).  In place (out == x) is supported: every element is read and
 * written by the same thread.  Any other overlap of out with x or f is the caller's error. */
typedef struct {
    const double* x;
    const double* f;
    double* out;
    int64_t outer, axis, inner;
} cyb_scale_axis_desc;
int cyb_scale_axis_batched_f64(cyb_ctx_t ctx, const cyb_scale_axis_desc* descs, int64_t n);

/* Gather (apply_mask, numpy.cpp:605-613) / scatter-into-zeros (enlarge_leg, numpy.cpp:700-728)
 * along one axis of a block viewed as (outer, axis, inner).  idx (device, int64) lists the kept
 * positions (n_keep entries).  gather: out(outer,n_keep,inner) = x(outer, idx[j], inner);
 * scatter: out(outer,axis,inner) = 0 except out(:, idx[j], :) = x(:, j, :). */
typedef struct {
    const double* x;
    double* out;
    const int64_t* idx;
    int64_t outer, axis, inner, n_keep;
} cyb_mask_desc;
int cyb_mask_gather_batched_f64(cyb_ctx_t ctx, const cyb_mask_desc* descs, int64_t n);
int cyb_mask_scatter_batched_f64(cyb_ctx_t ctx, const cyb_mask_desc* descs, int64_t n);

/* ---- complex128 on the tdot path ------------------------------------------------------------------
 * The reference's blocks are float64 or complex128 (Dtype, include/cyten/block_backend/dtypes.h; numpy.cpp
 * dispatches every virtual on it).  Complex blocks are stored interleaved (re, im) as numpy does.  A complex
 * product runs through the same real grouped GEMM: A is read in place as a real M x 2K matrix, C written in place
 * as a real M x 2N matrix, and B is expanded once into the real 2K x 2N matrix [[br, bi], [-bi, br]] per element
 * (cyb_complex_expand_batched_f64).  Decompositions of complex blocks: the *_c128 entries further down. */
typedef struct cyb_cexpand_desc {
    const double* src; /* complex K x N view, element (k, n) at src + 2*(k*rs + n*cs); 16-byte aligned */
    int64_t rs, cs;    /* strides in complex elements */
    int64_t K, N;
    double* dst;       /* 2K x 2N doubles, row-major, contiguous; 16-byte aligned.  A src or dst that is not
                          16-byte aligned is refused with CYB_ERR_INVALID (unless K * N == 0) */
} cyb_cexpand_desc;
int cyb_complex_expand_batched_f64(cyb_ctx_t ctx, const cyb_cexpand_desc* descs, int64_t n);
/* out = a*x + b*y on complex vectors of desc.n complex elements (y may be NULL): Block::operator+ / mul /
 * linear_combination for complex128 (numpy.cpp:1358-1365) */
/* elementwise functions of complex vectors (desc.n complex elements; x, y interleaved complex): op 0 |z| and
 * 4 angle write desc.n doubles to out; 1 sqrt, 2 exp, 3 log, 5 z*w, 6 z/w write complex
 * (abs / sqrt / exp / log / angle numpy.cpp:449-456,1066-1073,730-737,862-869,587-594; Block::operator* /  :217-227).
 * NaN, Inf, signed zeros and arguments near the ends of the double range give numpy's results (C99 Annex G for sqrt /
 * exp / log; z*w rounds the products with Im z and fuses those with Re z like numpy's vectorised loop; z/0 divides each
 * part by +0).  A quotient by a non-zero divisor whose parts are both denormal is computed directly (numpy overflows). */
int cyb_elementwise_batched_c128(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, int32_t op);
int cyb_axpby_batched_c128(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n,
                           double a_re, double a_im, double b_re, double b_im);
/* result_dev[0] = re, result_dev[1] = im of sum over all list entries of sum_i conj(x_i) * y_i; x, y interleaved
 * complex, desc.n counts complex elements (`out` unused).  Deterministic two-stage reduction: bit-identical from run to
 * run.  The inner product of complex Krylov vectors and of complex block lists (abelian.cpp:2159-2211). */
int cyb_dot_batched_c128(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n, double* result_dev);

/* ---- projections against a list of m <= 64 basis vectors (GMRES and the projected operator) ----------------------------
 * basis: a HOST array of m device pointers, each a contiguous vector of n elements (f64: doubles; c128: interleaved complex,
 * n counts complex elements, 16-byte aligned); w: a contiguous vector of the same kind.  Coefficients are device arrays of m
 * doubles (f64) or m interleaved complex numbers (c128).  Enqueued on the context stream with no host synchronisation;
 * fixed work split for a given (n, m), fixed summation order: bit-identical from run to run.  m > 64: CYB_ERR_UNSUPPORTED.
 *
 * multi-dot: h_dev[j] = sum_i conj(V_j[i]) w[i], w read once -- the coefficients of ProjectedLinearOperator with
 * project_operator=False (sparse.cpp:302-306). */
int cyb_multi_dot_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* w, int64_t n, double* h_dev);
int cyb_multi_dot_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* w, int64_t n, double* h_dev);
/* multi-axpy: w += alpha * sum_j h_dev[j] V_j, h read from device memory -- the penalty term of ProjectedLinearOperator
 * (sparse.cpp:316-321). */
int cyb_multi_axpy_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* h_dev, double alpha, double* w, int64_t n);
int cyb_multi_axpy_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* h_dev, double alpha_re, double alpha_im,
                        double* w, int64_t n);
/* classical Gram-Schmidt step, passes 1 or 2 (CGS2): w <- (1 - V V^H)^passes w in place.  out_dev receives the coefficients
 * summed over the passes (m doubles, or 2m for c128: the Hessenberg column of GMRES::arnoldi, krylov_based.cpp:453-469)
 * followed by |w| after the last update (one double). */
int cyb_gram_schmidt_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, double* w, int64_t n, int32_t passes, double* out_dev);
int cyb_gram_schmidt_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, double* w, int64_t n, int32_t passes, double* out_dev);
/* The same reductions with a weight per granule of 256 elements (doubles in the f64 form, complex numbers in the c128 form):
 * h_j = sum_i d(i) conj(V_j[i]) w[i] and |w| = sqrt(sum_i d(i) |w[i]|^2) with d(i) = weights_dev[i / 256]; the update
 * w <- w - sum_j h_j V_j is unweighted.  weights_dev: ceil(n / 256) device doubles -- the quantum dimension of the coupled
 * sector a fusion-tree pool keeps in that granule (FusionTreeBackend::inner / ::norm, fusion_tree_backend.cpp:1238-1296).
 * Same work split, same summation order and same error rules as the unweighted entries; a NULL table with n > 0 is
 * CYB_ERR_INVALID; m == 0 in the Gram-Schmidt step still writes the weighted norm. */
int cyb_multi_dot_weighted_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* w, int64_t n, const double* weights_dev,
                               double* h_dev);
int cyb_multi_dot_weighted_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, const double* w, int64_t n, const double* weights_dev,
                                double* h_dev);
int cyb_gram_schmidt_weighted_f64(cyb_ctx_t ctx, const double* const* basis, int64_t m, double* w, int64_t n, int32_t passes,
                                  const double* weights_dev, double* out_dev);
int cyb_gram_schmidt_weighted_c128(cyb_ctx_t ctx, const double* const* basis, int64_t m, double* w, int64_t n, int32_t passes,
                                   const double* weights_dev, double* out_dev);
/* Orthonormalises a LIST in place (gram_schmidt(vecs, rcond), sparse.cpp:420-436) with no host wait between its steps.
 * vecs: a HOST array of m <= 64 device pointers to contiguous vectors of n elements, alignment and n as above.  For
 * k = 0 .. m-1: the CGS2 step above (passes = 2) of vecs[k] against vecs[0..k-1], then one streaming pass that reads the
 * norm the step left on the device: norm > rcond (false for NaN) multiplies every element by the double 1.0 / norm (both
 * parts of a complex one), anything else WRITES +0.0 over the vector, so that a dropped vector -- whatever it held --
 * contributes exactly nothing to the later steps.  out_dev: 2m device doubles, out[k] the norm, out[m + k] 1.0 (kept) or
 * 0.0 (dropped).  The weighted forms take the norms and coefficients with the granule table of the weighted entries.
 * m == 0 or n == 0: nothing is launched, out_dev is not written; m > 64: CYB_ERR_UNSUPPORTED. */
int cyb_orthonormalize_f64(cyb_ctx_t ctx, double* const* vecs, int64_t m, int64_t n, double rcond, double* out_dev);
int cyb_orthonormalize_c128(cyb_ctx_t ctx, double* const* vecs, int64_t m, int64_t n, double rcond, double* out_dev);
int cyb_orthonormalize_weighted_f64(cyb_ctx_t ctx, double* const* vecs, int64_t m, int64_t n, double rcond, const double* weights_dev,
                                    double* out_dev);
int cyb_orthonormalize_weighted_c128(cyb_ctx_t ctx, double* const* vecs, int64_t m, int64_t n, double rcond, const double* weights_dev,
                                     double* out_dev);
/* Basis rotation of thick-restart Lanczos, Y = V S in ONE streaming pass: dst[i][p] = sum_{j<m} q[j * k + i] * src[j][p] for
 * i < k, p < n.  src / dst: HOST arrays of m <= 64 / k <= 32 device pointers to contiguous vectors of n doubles (8-byte
 * aligned; 16-byte accesses when every pointer is 16-byte aligned).  q_host: m x k row-major doubles in HOST memory, uploaded
 * through the context's ring (no allocation, no host wait).  One thread per position, j ascending, no atomics: bit-identical
 * from run to run and whatever the alignment.  A dst[i] may BE any src[j] (in place, dst[i] = src[i], or any other
 * assignment): a thread loads all m values of its positions before it stores any of its k results and touches no other
 * position.  Two equal dst entries, or a dst range that overlaps another dst or a src range only partly: CYB_ERR_INVALID,
 * as are m > 64, k > 32, a NULL table or entry and a pointer that is not 8-byte aligned; nothing is launched then.
 * m == 0, k == 0 or n == 0: success, nothing is launched.  V (m n words) is read once and Y (k n words) written once.
 * complex128 pools need no second entry: the small matrix is real (the Ritz vectors of a real symmetric tridiagonal or arrow
 * matrix), so a pool of n complex numbers is rotated as 2n doubles.  There is no weighted form: the rotation is linear, and
 * the zero gaps of a pool stay zero. */
int cyb_basis_rotate_f64(cyb_ctx_t ctx, const double* const* src, int64_t m, double* const* dst, int64_t k, const double* q_host,
                         int64_t n);

/* ---- host-side sector matching of a contraction (no device work) ------------------------------------------------
 * The int64 bookkeeping of abelian_compose_worker (src/backends/abelian.cpp:1239-1469) in C++, as in the reference:
 * contracts the last `num_contr` legs of a with the first `num_contr` legs of b (a.legs[na_legs - 1 - i] pairs with
 * b.legs[i]).  Block tables are row-major int64 (one row per block, one column per leg, entries = sector index on that
 * leg); a leg is its sorted sector charges (n_sectors x n_sym), multiplicities and orientation sign; moduli[k] = 0 for a
 * U(1) factor, N for Z_N.  The plan lists, per result block (rows lexsorted with the last column as primary key, like
 * BlockInds::lexsort_indices), its sector indices, its shape and the (a-block, b-block) pairs whose products are summed:
 * pairs of result g are pair_a/pair_b[group_offsets[g] .. group_offsets[g + 1]).  flops = sum 2 M N K. */
typedef struct {
    int64_t n_sectors;
    const int64_t* sectors; /* n_sectors x n_sym */
    const int64_t* mults;   /* n_sectors */
    int32_t sign;           /* +1 / -1 */
    int32_t pad;
} cyb_leg;
typedef struct cyb_compose_plan_s* cyb_compose_plan_t;
int cyb_compose_plan_create(const int64_t* moduli, int32_t n_sym, const cyb_leg* a_legs, int32_t na_legs,
                            const int64_t* a_block_inds, int64_t na_blocks, const cyb_leg* b_legs, int32_t nb_legs,
                            const int64_t* b_block_inds, int64_t nb_blocks, int32_t num_contr, cyb_compose_plan_t* out);
int cyb_compose_plan_sizes(cyb_compose_plan_t plan, int64_t* n_res, int64_t* n_pairs, int64_t* n_cols);
int cyb_compose_plan_get(cyb_compose_plan_t plan, int64_t* res_block_inds, int64_t* res_shapes, int64_t* group_offsets,
                         int64_t* pair_a, int64_t* pair_b, double* flops);
/* The hot loop of abelian_compose_worker (src/backends/abelian.cpp:1424-1460: matrix_dot + operator+ per matched pair,
 * reshape of the result) for operand blocks that are C-contiguous float64 arrays: the descriptors of the grouped GEMM are
 * built inside the library from the plan and three address tables, and ONE asynchronous launch is enqueued on the context's
 * stream.  a_ptrs[i] / b_ptrs[j]: device addresses of a's i-th / b's j-th block (the block-table order the plan was created
 * with; with more than one contracted leg the b-blocks must hold their contracted axes in a's reversed order, as
 * abelian.cpp:1349-1382 permutes them).  which: indices of the plan's result blocks to compute (n_which of them; NULL = all,
 * in plan order) -- a rank of a sharded contraction computes its own sectors only; out_ptrs[k]: address of the M x N result
 * of which[k].  flops / bytes (may be NULL): algorithmic 2 M N K and 8 (M K + K N + M N) sums of what was enqueued. */
int cyb_compose_plan_enqueue_f64(cyb_ctx_t ctx, cyb_compose_plan_t plan, const int64_t* a_ptrs, const int64_t* b_ptrs,
                                 const int64_t* which, int64_t n_which, const int64_t* out_ptrs, double* flops, double* bytes);
int cyb_compose_plan_destroy(cyb_compose_plan_t plan);

/* ---- complex128 decompositions -----------------------------------------------------------------------------------
 * Same descriptors as the float64 entries, every matrix pointer addressing interleaved (re, im) storage and every
 * leading dimension counted in complex elements; S and W stay real.  Blocks with min(m, n) <= 64, max(m, n) <= 128 and
 * 32 * (Np * (max | 1) + Np * (Np | 1)) <= 150 KB (Np = min rounded up to even; e.g. 64 x 64, 48 x 96, 40 x 128): one
 * workgroup per block runs a complex one-sided Jacobi iteration in LDS (csrc/csvd_small.hip).  Larger blocks: the same
 * iteration with the work matrix in device memory, one launch per tournament round for all blocks of the call, null
 * directions of rank-deficient blocks completed block-wise (csrc/csvd_large.hip; plain FMA arithmetic, not the MFMA
 * block engine of the float64 path).  info[i] = sweeps used.
 * NumpyBlockBackend::matrix_svd / eigh on complex128 blocks (numpy.cpp:1247-1297, 658-680). */
int cyb_svd_batched_c128(cyb_ctx_t ctx, const cyb_svd_desc* descs, int64_t n, int32_t* info);
int cyb_eigh_batched_c128(cyb_ctx_t ctx, const cyb_eigh_desc* descs, int64_t n, int32_t* info);
/* QR of complex128 blocks (scipy.linalg.qr economic / full, numpy.cpp:1236-1245: LAPACK zgeqrf + zungqr): Householder
 * reflections built as zlarfg builds them (csrc/cqr_house.hip) -- one workgroup per block for blocks of at most 96 x 96
 * elements, one launch per column step for the whole list beyond.  Backward stable for every block (rank deficient,
 * copied or zero columns, graded); Q unitary, R upper triangular with a real non-negative diagonal (row j of R and column
 * j of Q carry the sign of LAPACK's beta_j, so scipy's R agrees up to the signs of its rows). */
int cyb_qr_batched_c128(cyb_ctx_t ctx, const cyb_qr_desc* descs, int64_t n);

/* ---- linear combinations of strided views ------------------------------------------------
 * dst[idx] = (accumulate ? dst[idx] : 0) + sum_{t in [term_begin, term_end)} coeff_t * src_t[idx]  for idx over `shape`,
 * all strides in elements.  One launch for the tree-block updates of FusionTreeBackend::apply_instructions
 * (src/backends/fusion_tree_backend.cpp:593-631): TreePairMapping::transform_tensor
 * (src/backends/fusion_tree_mapping.cpp:391-513) builds `tree_block = sum_I f_JI * old_block[slice_I]`
 * (:447-468: get_item, mul, Block::operator+), applies permute_combined_matrix (:491-492) and stores
 * `new_block[slices] = permuted` (:493-497) once per (tree pair, term); here the permutation lives in the source
 * strides and the placement in the destination view.  Destinations of one call must not overlap. */
typedef struct {
    double* dst;
    int32_t ndim;
    int32_t accumulate;
    int32_t term_begin, term_end;
    int64_t shape[CYB_MAX_NDIM];
    int64_t dst_strides[CYB_MAX_NDIM];
} cyb_lincomb_desc;
typedef struct {
    const double* src;
    double coeff;
    int64_t src_strides[CYB_MAX_NDIM];
} cyb_lincomb_term;
int cyb_lincomb_strided_batched_f64(cyb_ctx_t ctx, const cyb_lincomb_desc* descs, int64_t n, const cyb_lincomb_term* terms,
                                    int64_t n_terms);
/* complex128 form of the same: `dst` and the sources are interleaved (re, im) arrays, shapes / strides count complex
 * elements, coefficients are complex -- every anyonic R / C / B symbol is (tests/python_tests/backends/
 * test_fusion_tree_backend.py:59-71).  A term with src_real != 0 reads a float64 source (strides in doubles): real data
 * under a complex mapping, the `dtype = to_complex(dtype)` of fusion_tree_mapping.cpp:433-436. */
typedef struct {
    const double* src;
    double coeff_re, coeff_im;
    int32_t src_real;
    int32_t reserved;
    int64_t src_strides[CYB_MAX_NDIM];
} cyb_lincomb_term_c128;
int cyb_lincomb_strided_batched_c128(cyb_ctx_t ctx, const cyb_lincomb_desc* descs, int64_t n, const cyb_lincomb_term_c128* terms,
                                     int64_t n_terms);

/* ---- grouped partial trace ------------------------------------------------------------------------------------
 * Every result block of AbelianBackend::partial_trace (src/backends/abelian.cpp:2954-3081) in ONE launch: replaces the
 * per-block block_backend->trace_partial (numpy.cpp:1166-1195: transpose + reshape + trace, a copy of the whole block) and
 * the Block::operator+ per further contribution to the same result block (abelian.cpp:3026-3029); also the Scalar case
 * (:3042-3055) and trace_full (:3595-3620).
 *   out[r] = sum_{t in [first_term, first_term + n_terms)} sum_tau src_t[r . rem_strides_t + tau . pair_stride_t]
 * for r over `shape` (C order; dst is C-contiguous over these remaining axes) and tau over the pair extents of term t.
 * pair_stride[p] is the SUM of the source strides of the two traced axes of pair p, so that walking it walks the diagonal
 * of the pair.  All strides count elements; sources are read in place as strided views.  ndim + 2 * n_pairs <=
 * CYB_MAX_NDIM.  Entries of pair_extent / pair_stride beyond n_pairs and of shape / rem_strides beyond ndim are ignored.
 * An output with no terms is written as zero; zero extents and empty lists are valid.  Every output element is summed by
 * one owner in a fixed order (terms ascending, tau with pair 0 fastest; tree shapes fixed): no atomics, no zero fill,
 * bit-identical from run to run.  The owner -- one lane, one wave or one workgroup -- is chosen per output record from
 * its element count and its number of addends (csrc/trace_grouped.hip).  The c128 entry reads and writes interleaved
 * (re, im) storage, strides counted in complex elements. */
#define CYB_TRACE_MAX_PAIRS 4
typedef struct {
    double* dst;
    int32_t ndim;     /* number of remaining axes */
    int32_t reserved;
    int64_t first_term, n_terms;
    int64_t shape[CYB_MAX_NDIM];
} cyb_trace_out;
typedef struct {
    const double* src;
    int32_t n_pairs;
    int32_t reserved;
    int64_t rem_strides[CYB_MAX_NDIM];
    int64_t pair_extent[CYB_TRACE_MAX_PAIRS];
    int64_t pair_stride[CYB_TRACE_MAX_PAIRS];
} cyb_trace_term;
int cyb_trace_grouped_f64(cyb_ctx_t ctx, const cyb_trace_out* outs, int64_t n_outs, const cyb_trace_term* terms, int64_t n_terms);
int cyb_trace_grouped_c128(cyb_ctx_t ctx, const cyb_trace_out* outs, int64_t n_outs, const cyb_trace_term* terms, int64_t n_terms);

/* ---- weighted partial trace into strided tiles ------------------------------------------------------------------
 * Every result block of FusionTreeBackend::partial_trace (src/backends/fusion_tree_backend.cpp:2883-3183) in ONE launch:
 * step 2 of it (:3092-3159) makes, per pair of tree blocks, get_item, reshape, trace_partial, reshape, mul by the B-symbol
 * factor (:3149), get_item of the destination tile, operator+ and set_item.  Here an output record is one destination tile
 * and a term record one contributing old tree pair:
 *   out[r] = sum_{t in [first_term, first_term + n_terms)} c_t * ( sum_tau src_t[r . rem_strides_t + tau . pair_stride_t] )
 *   written to dst + r . dst_strides, r over `shape` (ndim remaining axes), tau over the pair extents of term t.
 * The destination is a strided N-d view: in practice a tile rows x cols of a coupled block, the row range split into the
 * remaining codomain multiplicities, the column range into the remaining domain ones, with the block's leading dimension.
 * pair_stride[p] is the SUM of the two source strides of traced pair p (walking it walks the diagonal), ndim + 2 * n_pairs
 * <= CYB_MAX_NDIM, entries beyond ndim / n_pairs are ignored -- the meanings of cyb_trace_term.  c_t = coeff_re + i coeff_im.
 *   * Every output element has exactly one owner, which adds its terms in ascending order (tau with pair 0 fastest, tree
 *     shapes fixed): no float atomics, no zero fill, no second pass; results are bit-identical from run to run.
 *   * An output with no terms is written as zeros: a tile nothing contributes to is zeroed without a memset.
 *   * The coefficient multiplies a term's sum once per output element, not once per addend.
 *   * Sources are read in place and may overlap each other.  Destination tiles of one call must not overlap; the caller
 *     vouches for that.  Zero extents and empty lists are valid.
 *   * src_real != 0 (c128 entry only; the f64 entry ignores it): the source is float64 data read in place, strides in
 *     doubles -- a real tensor under complex B symbols needs no promotion pass (as cyb_lincomb_term_c128).  The c128 entry
 *     reads and writes interleaved (re, im) storage otherwise, strides counted in complex elements.
 *   * The f64 entry requires coeff_im == 0 of every term: else CYB_ERR_INVALID, nothing is launched.
 *   * Everything is validated on the host before anything is uploaded or launched: ndim, pair counts, term ranges,
 *     negative extents, NULL pointers of non-empty outputs / terms.  A refused call leaves the context as it found it.
 * The owner -- one lane, one wave or one workgroup -- is chosen per output record from its element count and its number of
 * addends (csrc/tree_trace.hip). */
typedef struct {
    double* dst;
    int32_t ndim;     /* number of remaining axes */
    int32_t reserved;
    int64_t first_term, n_terms;
    int64_t shape[CYB_MAX_NDIM];
    int64_t dst_strides[CYB_MAX_NDIM];
} cyb_trace_weighted_out;
typedef struct {
    const double* src;
    double coeff_re, coeff_im;
    int32_t src_real;
    int32_t n_pairs;
    int64_t rem_strides[CYB_MAX_NDIM];
    int64_t pair_extent[CYB_TRACE_MAX_PAIRS];
    int64_t pair_stride[CYB_TRACE_MAX_PAIRS];
} cyb_trace_weighted_term;
int cyb_trace_weighted_f64(cyb_ctx_t ctx, const cyb_trace_weighted_out* outs, int64_t n_outs, const cyb_trace_weighted_term* terms,
                           int64_t n_terms);
int cyb_trace_weighted_c128(cyb_ctx_t ctx, const cyb_trace_weighted_out* outs, int64_t n_outs, const cyb_trace_weighted_term* terms,
                            int64_t n_terms);

/* ---- weighted Kronecker products into strided tiles ---------------------------------------------------------------
 * Every result block of FusionTreeBackend::outer (src/backends/fusion_tree_backend.cpp:2609-2667) in ONE launch: the
 * reference makes, per (tree pair of a, tree pair of b), outer, permute_axes, combine_legs and then get_item, mul, operator+
 * and set_item per (new codomain tree, new domain tree) into a zero-filled result.  Here an output record is one destination
 * tile of ha * hb rows and wa * wb columns and a term record one contributing (tree pair of a, tree pair of b):
 *   dst[(ra * hb + rb) * ldd + ca * wb + cb] = sum_{t in [first_term, first_term + n_terms)} c_t * A_t[ra * a_rs + ca * a_cs]
 *                                                                                              * B_t[rb * b_rs + cb * b_cs]
 * ra < ha, rb < hb, ca < wa, cb < wb (the axes (a.cod, b.cod | a.dom, b.dom) in C order, :2636-2639), c_t = coeff_re + i coeff_im.
 * The destination tile has unit column stride; ldd is the leading dimension of the coupled block it lies in.  a_rs, a_cs,
 * b_rs, b_cs are row and column strides in elements of the operand's own type: views and transposed views are read in
 * place.  All terms of an output share its four extents.
 *   * Every destination element has exactly one owner, which adds its terms in ascending order as (c_t * A_t) * B_t: no
 *     float atomics, no zero fill, no second pass; results are bit-identical from run to run.
 *   * An output with no terms is written as zeros: a tile nothing contributes to is zeroed without a memset.
 *   * Zero extents and empty lists are valid.
 *   * Sources are read in place and may overlap each other.  Destination tiles of one call must not overlap; the caller
 *     vouches for that.
 *   * a_real / b_real != 0 (c128 entry only; the f64 entry ignores them): the operand is float64 data read in place, strides
 *     in doubles -- a real operand beside a complex one, or under complex amplitudes, needs no promotion pass.  The c128
 *     entry reads and writes interleaved (re, im) storage otherwise, strides and ldd counted in complex elements.
 *   * The f64 entry requires coeff_im == 0 of every term: else CYB_ERR_INVALID, nothing is launched.
 *   * Everything is validated on the host before anything is uploaded or launched: negative extents (and extents beyond
 *     2^30), term ranges, ldd < wa * wb of a tile of more than one row, NULL dst / a / b of a non-empty output.  A refused
 *     call returns CYB_ERR_INVALID with a message and leaves the context as it found it.
 * One wave owns a work item of a record, lanes along the columns, 16-byte stores (csrc/tree_outer.hip). */
typedef struct {
    double* dst;
    int64_t ha, hb, wa, wb;
    int64_t ldd;
    int64_t first_term, n_terms;
} cyb_outer_weighted_out;
typedef struct {
    const double* a;
    const double* b;
    double coeff_re, coeff_im;
    int32_t a_real, b_real;
    int64_t a_rs, a_cs, b_rs, b_cs;
} cyb_outer_weighted_term;
int cyb_outer_weighted_f64(cyb_ctx_t ctx, const cyb_outer_weighted_out* outs, int64_t n_outs, const cyb_outer_weighted_term* terms,
                           int64_t n_terms);
int cyb_outer_weighted_c128(cyb_ctx_t ctx, const cyb_outer_weighted_out* outs, int64_t n_outs, const cyb_outer_weighted_term* terms,
                            int64_t n_terms);

/* ---- weighted short contractions into strided tiles ---------------------------------------------------------------
 * Every result block of FusionTreeBackend::partial_compose (src/backends/fusion_tree_backend.cpp:2670-2880) in ONE launch:
 * the reference makes, per (outer tree, b codomain tree, b domain tree, old tree, new tree), get_item, reshape, tdot,
 * permute_axes, reshape, as_scalar, get_item, mul, operator+ and set_item into a zero-filled result.  Here an output record
 * is one destination tile seen as the 4-level index space (x0, x1, x2, x3) in C order, x_l < ext[l], with the destination
 * strides sd[4]; the level `axis` (1 or 2) carries the surviving index n of b.  A term record is one contributing (old tree,
 * b tree pair) with its own contracted extent K:
 *   dst[sum_l x_l * sd[l]] = sum_{t in [first_term, first_term + n_terms)} c_t * sum_{k < K_t}
 *                                A_t[sum_{l != axis} x_l * sa[l] + k * sa[axis]] * B_t[x_axis * b_ns + k * b_ks]
 * c_t = coeff_re + i coeff_im.  All strides count elements of the operand's own type: views and transposed views are read in
 * place.  The two cases of the reference, with m0 / m2 the products of the multiplicities before / after the inserted leg,
 * N = ext[axis], lda / ldd the leading dimensions of the coupled blocks:
 *   contraction in a's domain (:2797-2827): levels (r, i0, n, i2), axis = 2, sd = (ldd, N m2, m2, 1), sa = (lda, K m2, m2, 1),
 *       B the K x N tree block (b_ks its row stride, b_ns its column stride);
 *   contraction in a's codomain (:2828-2857): levels (i0, n, i2, col), axis = 1, sd = (N m2 ldd, m2 ldd, ldd, 1),
 *       sa = (K m2 lda, m2 lda, lda, 1), B the N x K tree block (b_ns its row stride, b_ks its column stride).
 *   * Every destination element has exactly one owner.  Within a term it sums k ascending, then adds c_t * that sum, terms
 *     ascending: no float atomics, no zero fill, no second pass; results are bit-identical from run to run.
 *   * An output with no terms is written as zeros.
 *   * Zero extents, K == 0 (the term adds nothing; its a and b are not read and may be NULL) and empty lists are valid.
 *   * Sources are read in place and may overlap each other.  Destination tiles of one call must not overlap; the caller
 *     vouches for that.
 *   * a_real / b_real != 0 (c128 entry only; the f64 entry ignores them): the operand is float64 data read in place, strides
 *     in doubles -- a real operand beside a complex one needs no promotion pass.  The c128 entry reads and writes
 *     interleaved (re, im) storage otherwise, strides counted in complex elements.
 *   * The f64 entry requires coeff_im == 0 of every term: else CYB_ERR_INVALID, nothing is launched.
 *   * Everything is validated on the host before anything is uploaded or launched: negative extents, extents or K beyond
 *     2^30 (or negative K), axis outside {1, 2}, term ranges, sd[3] != 1 where ext[3] > 1, NULL dst of a non-empty output,
 *     NULL a / b of a term with K > 0 of a non-empty output.  A refused call returns CYB_ERR_INVALID with a message and leaves
 *     the context as it found it.
 * One wave owns a work item of a record, lanes along the flat order of the levels.  16-byte stores: one complex, or a pair
 * of doubles (x_p, x_p + 1) along the last level p whose extent is above 1, iff sd[p] == 1, ext[p] is even, sd[l] is even for
 * every l < p with ext[l] > 1, and dst is 16-byte aligned; else one double per lane.  Iff p != axis, n runs in the registers of a
 * lane (four values at a time, A loaded once per k for all of them) instead of in the lanes (csrc/tree_compose.hip).  The kernel is
 * shaped for small K and N (multiplicities of physical / MPO legs); a large K is correct but runs at no GEMM rate. */
typedef struct {
    double* dst;
    int64_t ext[4];
    int64_t sd[4];
    int32_t axis;     /* 1 or 2: the level of b's surviving index n */
    int32_t reserved;
    int64_t first_term, n_terms;
} cyb_compose_weighted_out;
typedef struct {
    const double* a;
    const double* b;
    double coeff_re, coeff_im;
    int32_t a_real, b_real;
    int64_t K;
    int64_t sa[4];
    int64_t b_ns, b_ks;
} cyb_compose_weighted_term;
int cyb_compose_weighted_f64(cyb_ctx_t ctx, const cyb_compose_weighted_out* outs, int64_t n_outs, const cyb_compose_weighted_term* terms,
                             int64_t n_terms);
int cyb_compose_weighted_c128(cyb_ctx_t ctx, const cyb_compose_weighted_out* outs, int64_t n_outs, const cyb_compose_weighted_term* terms,
                              int64_t n_terms);

/* ---- fusion-tree tensors <-> dense arrays ---------------------------------------------------------------------------
 * FusionTreeBackend::to_dense_block (src/backends/fusion_tree_backend.cpp:1856-1973 with _get_forest_block_contribution
 * :1532-1604) and ::from_dense_block (:1680-1853 with _add_forest_block_entries :1606-1677) in ONE launch each: the reference
 * makes, per pair of trees of every forest pair, zeros, two to_dense_block of trees, tdot, get_item, reshape, outer and
 * operator+, then permute_axes, reshape and an accumulating set_item into a zero-filled dense tensor (forward), and two
 * tdot, trace_partial, a division, reshape and set_item (backward).
 *
 * to_dense: an output record is one region of the dense tensor (the positions of one combination of uncoupled sectors),
 * seen as the index space of n_levels <= CYB_TREE_DENSE_MAX_LEVELS levels x_l < ext[l] in C order (the last level is the
 * fastest; the lanes of a wave run along it) -- one (k, m) pair per leg, k inside the sector's dimension, m inside its
 * multiplicity, in whatever order makes the last level the contiguous run of the destination.  A term record is one
 * contributing (coupled block, tree alpha, tree beta):
 *   dst[sum_l x_l sd[l]] = sum_{t in [first_term, first_term + n_terms)} S[s_off_t + sum_l x_l ss[l]]
 *                              * B_t[(first_row_t + sum_l x_l sr[l]) * rs_t + (first_col_t + sum_l x_l sc[l]) * cs_t]
 * S = s_table is ONE device table that holds the contracted tree-tensor pairs S_{alpha beta}[k_a..., k_b...] of the call (a
 * small tensor per term, not a scalar); ss is nonzero on the k levels, sr / sc on the m levels of the codomain / domain legs.
 * from_dense: an output record is one tile (tree alpha, tree beta) of a coupled block with n_levels <= CYB_TREE_DENSE_MAX_LEGS
 * levels (m..., n...), in whatever order makes the last level the contiguous run of the source; a term is one dense region:
 *   dst[sum_l x_l sd[l]] = (sum_t sum_{k} conj(S[s_off_t + k]) * A_t[sum_l x_l ss[l] + sum_j k_j ks[j]]) / divisor
 * k = (k_0, .., k_{n_k - 1}), k_j < kext[j], counted in C order; summed k ascending inside the lane, divided after the sum.
 *   * Every destination element has exactly one owner, which adds its terms in ascending order in registers: no float
 *     atomics, no zero fill, no second pass; results are bit-identical from run to run.
 *   * An output with no terms is written as zeros.  Zero extents and empty lists are valid.
 *   * All strides count elements of the operand's own type and may be negative or zero; blocks, regions and the table are read in place
 *     and may overlap each other.  Destinations of one call must not overlap; the caller vouches for that, and for
 *     every address the strides reach.
 *   * block_real / src_real / s_real != 0 (c128 entries only; the f64 entries ignore them): the operand is float64 data read
 *     as it stands, offsets in doubles -- a real block under complex tree tensors (or the reverse) needs no promotion pass.
 *     The c128 entries read and write interleaved (re, im) storage otherwise.
 *   * Everything is validated on the host before anything is uploaded or launched: level counts, negative extents (and
 *     extents beyond 2^30), term ranges, negative first_row / first_col / s_off, a zero or NaN divisor, NULL dst / block /
 *     src / s_table of a non-empty output.  A refused call returns CYB_ERR_INVALID with a message and leaves the context as it
 *     found it.
 * One wave owns a work item of a record; a lane holds one element (csrc/tree_dense.hip). */
#define CYB_TREE_DENSE_MAX_LEGS 6
#define CYB_TREE_DENSE_MAX_LEVELS 12
typedef struct {
    double* dst;
    int32_t n_levels;
    int32_t reserved;
    int64_t ext[CYB_TREE_DENSE_MAX_LEVELS];
    int64_t sd[CYB_TREE_DENSE_MAX_LEVELS]; /* destination stride */
    int64_t ss[CYB_TREE_DENSE_MAX_LEVELS]; /* stride into S */
    int64_t sr[CYB_TREE_DENSE_MAX_LEVELS]; /* what the level adds to the row index of the block */
    int64_t sc[CYB_TREE_DENSE_MAX_LEVELS]; /* ... to the column index */
    int64_t first_term, n_terms;
} cyb_tree_to_dense_out;
typedef struct {
    const double* block;
    int64_t first_row, first_col;
    int64_t rs, cs; /* row and column stride of the block: (ld, 1), or (1, ld) of a transposed view */
    int64_t s_off;
    int32_t block_real, s_real;
} cyb_tree_to_dense_term;
typedef struct {
    double* dst;
    int32_t n_levels;
    int32_t n_k;
    int64_t ext[CYB_TREE_DENSE_MAX_LEGS];
    int64_t sd[CYB_TREE_DENSE_MAX_LEGS];   /* destination stride */
    int64_t ss[CYB_TREE_DENSE_MAX_LEGS];   /* source stride of the same level */
    int64_t kext[CYB_TREE_DENSE_MAX_LEGS]; /* the contracted levels */
    int64_t ks[CYB_TREE_DENSE_MAX_LEGS];   /* their source strides */
    double divisor;
    int64_t first_term, n_terms;
} cyb_tree_from_dense_out;
typedef struct {
    const double* src; /* the first element of the region */
    int64_t s_off;
    int32_t src_real, s_real;
} cyb_tree_from_dense_term;
int cyb_tree_to_dense_f64(cyb_ctx_t ctx, const cyb_tree_to_dense_out* outs, int64_t n_outs, const cyb_tree_to_dense_term* terms, int64_t n_terms,
                          const double* s_table);
int cyb_tree_to_dense_c128(cyb_ctx_t ctx, const cyb_tree_to_dense_out* outs, int64_t n_outs, const cyb_tree_to_dense_term* terms, int64_t n_terms,
                           const double* s_table);
int cyb_tree_from_dense_f64(cyb_ctx_t ctx, const cyb_tree_from_dense_out* outs, int64_t n_outs, const cyb_tree_from_dense_term* terms,
                            int64_t n_terms, const double* s_table);
int cyb_tree_from_dense_c128(cyb_ctx_t ctx, const cyb_tree_from_dense_out* outs, int64_t n_outs, const cyb_tree_from_dense_term* terms,
                             int64_t n_terms, const double* s_table);

/* ---- grouped, weighted, strided window copies -----------------------------------------------------------------------
 * Every window of every result block of FusionTreeBackend::from_grid (src/backends/fusion_tree_backend.cpp:3375-3518) or
 * ::from_tree_pairs (:3186-3263) in ONE launch: the reference makes get_item, reshape, copy_block, reshape, get_item,
 * operator+, set_item, reshape and set_item per (grid entry, codomain forest, domain forest) into a zero-filled result
 * (from_grid), and permute_axes, reshape and set_item per tree pair into zeros (from_tree_pairs).  A record is one window of
 * a coupled block: h consecutive rows, nq runs of wn consecutive columns, one run every cp columns, in a block with the
 * leading dimension ldd; dst addresses its first element:
 *   dst[r * ldd + q * cp + w] = c * src[sum_l r_l * rs[l] + sum_l x_l * cs[l]]          r < h, q < nq, w < wn
 * r is counted in C order over the n_row_levels levels rext[] (their product is h), x = q * wn + w in C order over the
 * n_col_levels levels cext[] (their product is nq * wn); c = coeff_re + i coeff_im.
 *   * src == NULL: the window is written as zeros (levels, strides and the coefficient's value are not read) -- the cells of
 *     a result that nothing feeds are filled without a memset.
 *   * Source strides count elements of the source's own type and may be zero or negative.  Sources are read in place,
 *     transposed (dagger) views included, and may overlap each other.  The caller vouches for every address the strides reach.
 *   * src_real != 0 (c128 entry only; the f64 entry ignores it): the source is float64 data read as it stands, strides in
 *     doubles -- a real entry beside a complex one, or under a complex coefficient, needs no promotion pass.  The c128 entry
 *     reads and writes interleaved (re, im) storage otherwise; cp and ldd count complex elements.
 *   * The f64 entry requires coeff_im == 0 of every record: else CYB_ERR_INVALID, nothing is launched.
 *   * Windows of one call must not overlap; the caller vouches for that.  Every destination element has exactly one owner: no
 *     atomics, no second pass, results are bit-identical from run to run.
 *   * c == 1 copies bits exactly (-0.0, NaN payloads); any other c is one product per component pair, never an FMA with a
 *     zero addend.
 *   * Zero extents and n_recs == 0 are valid.  cp is not read where nq == 1, ldd not where h == 1.
 *   * Everything is validated on the host before anything is uploaded or launched: level counts, negative extents and
 *     extents beyond 2^30 (h, nq, wn and every level), the products of the levels against h and nq * wn (of a record with a
 *     source), cp < wn with nq > 1, ldd < (nq - 1) * cp + wn with h > 1, NULL dst of a non-empty window.  A refused call
 *     returns CYB_ERR_INVALID with a message and leaves the context as it found it.
 * One wave owns a work item of a record, its lanes on 64 consecutive elements of the window's C order (along a run, or
 * across several narrow runs and rows), 16-byte stores where every pair of the window is aligned (csrc/tree_place.hip). */
#define CYB_TREE_PLACE_MAX_LEVELS 6
typedef struct {
    double* dst;
    const double* src; /* NULL: zeros */
    int64_t h, nq, wn, cp, ldd;
    int32_t n_row_levels, n_col_levels;
    int64_t rext[CYB_TREE_PLACE_MAX_LEVELS], rs[CYB_TREE_PLACE_MAX_LEVELS];
    int64_t cext[CYB_TREE_PLACE_MAX_LEVELS], cs[CYB_TREE_PLACE_MAX_LEVELS];
    double coeff_re, coeff_im;
    int32_t src_real, reserved;
} cyb_tree_place_rec;
int cyb_tree_place_f64(cyb_ctx_t ctx, const cyb_tree_place_rec* recs, int64_t n_recs);
int cyb_tree_place_c128(cyb_ctx_t ctx, const cyb_tree_place_rec* recs, int64_t n_recs);

/* ---- grouped, weighted sums of strided windows ----------------------------------------------------------------------
 * Every strip of every result block of one side of a factorized fusion-tree move in ONE launch:
 * FactorizedTreeMapping::transform_splitting_trees / ::transform_fusion_trees (src/backends/fusion_tree_mapping.cpp:627-674,
 * :676-725) make get_item, mul and operator+ per (new tree, old tree), then permute_combined_idx and set_item per new tree,
 * into a zero-filled block.  An output record is one window of a result block, the window of cyb_tree_place_rec (h rows, nq
 * runs of wn columns, one run every cp columns, leading dimension ldd; dst addresses its first element), with ONE table of
 * source levels that all of its terms share; a term record is one source: a pointer, a coefficient and a base offset:
 *   dst[r * ldd + q * cp + w] = sum_t c_t * src_t[base_t + sum_l r_l * rs[l] + sum_l x_l * cs[l]]      r < h, q < nq, w < wn
 * r is counted in C order over the n_row_levels levels rext[] (their product is h), x = q * wn + w in C order over the
 * n_col_levels levels cext[] (their product is nq * wn); c_t = coeff_re + i coeff_im; t runs over first_term ..
 * first_term + n_terms - 1 of the term list.
 *   * An output with no terms is written as zeros (its levels and strides are not read): nothing needs a memset.
 *   * Every destination element has exactly one owner, which adds its terms in ascending order in registers: no atomics, no
 *     zero fill, no second pass; results are bit-identical from run to run.  The first term is assigned: an output with one
 *     term and c == 1 receives the bits of its source (-0.0, NaN payloads); any other c is one product per component pair.
 *   * Source strides and base count elements of the source's own type and may be zero or negative.  Sources are read in
 *     place, transposed views included, and may overlap each other.  The caller vouches for every address they reach.
 *   * src_real != 0 (c128 entry only; the f64 entry ignores it): the source is float64 data read as it stands, strides and
 *     base in doubles -- real data under a complex coefficient needs no promotion pass.  The c128 entry reads and writes
 *     interleaved (re, im) storage otherwise; cp and ldd count complex elements.
 *   * The f64 entry requires coeff_im == 0 of every term: else CYB_ERR_INVALID, nothing is launched.
 *   * Windows of one call must not overlap each other or a source; the caller vouches for that.
 *   * Zero extents and empty lists are valid.  cp is not read where nq == 1, ldd not where h == 1.
 *   * Everything is validated on the host before anything is uploaded or launched: level counts, term ranges, negative
 *     extents and extents beyond 2^30, the products of the levels against h and nq * wn (of an output with terms), cp < wn
 *     with nq > 1, ldd < (nq - 1) * cp + wn with h > 1, NULL dst of a non-empty window, NULL src of one of its terms.  A
 *     refused call returns CYB_ERR_INVALID with a message and leaves the context as it found it.
 * One wave owns a work item of a record; 16-byte stores where every pair of the window is aligned, one 16-byte load per pair
 * where the innermost source level has the stride 1 and every term is aligned, gathered loads where a permutation moves the
 * innermost level (csrc/tree_strip.hip). */
typedef struct {
    double* dst;
    int64_t h, nq, wn, cp, ldd;
    int32_t n_row_levels, n_col_levels;
    int64_t rext[CYB_TREE_PLACE_MAX_LEVELS], rs[CYB_TREE_PLACE_MAX_LEVELS];
    int64_t cext[CYB_TREE_PLACE_MAX_LEVELS], cs[CYB_TREE_PLACE_MAX_LEVELS];
    int64_t first_term, n_terms;
} cyb_tree_strip_out;
typedef struct {
    const double* src;
    double coeff_re, coeff_im;
    int32_t src_real, reserved;
    int64_t base; /* offset of the term's first element from src */
} cyb_tree_strip_term;
int cyb_tree_strip_f64(cyb_ctx_t ctx, const cyb_tree_strip_out* outs, int64_t n_outs, const cyb_tree_strip_term* terms, int64_t n_terms);
int cyb_tree_strip_c128(cyb_ctx_t ctx, const cyb_tree_strip_out* outs, int64_t n_outs, const cyb_tree_strip_term* terms, int64_t n_terms);

/* ---- grouped matrix exponential of small blocks ---------------------------------------------------------------------
 * E = exp(alpha * A) for every listed square matrix in ONE launch, one workgroup per matrix, the whole computation in LDS
 * (csrc/expm_small.hip).  Replaces NumpyBlockBackend::matrix_exp = scipy.linalg.expm (src/block_backend/numpy.cpp:1227-1234),
 * called once per diagonal block by AbelianBackend::act_block_diagonal_square_matrix (src/backends/abelian.cpp:562-593).
 * Algorithm: 1-norm of alpha * A; s = 0 if it is <= 1/2, else ceil(log2(norm / (1/2))); degree-18 Taylor polynomial of
 * alpha * A / 2^s in Horner form; s squarings -- the steps of HipBlockBackend.matrix_exp, with the same truncation bound
 * (< 2e-23).  Matrices are row-major; lda counts elements of the SOURCE type, lde elements of the result type.
 *   A == NULL: the zero matrix, E becomes the identity (a sector of a tensor that holds no block).
 *   a_is_real (c128 entry only): A addresses float64 data although E is complex -- a real Hamiltonian under
 *       alpha = -i dt needs no promotion pass.  The f64 entry reads and writes float64 and takes a real alpha.
 *   n == 0: the entry is skipped.  n above CYB_EXPM_SMALL_MAX_N_*: CYB_ERR_INVALID, nothing is launched (the caller runs such
 *       blocks on the grouped GEMM, see HipBlockBackend.matrix_exp_many).
 * The limits are what two n x n matrices (row length n | 1) take of one workgroup's LDS next to a 16 x 16 thread grid with
 * at most 6 x 6 (f64) / 4 x 4 (c128) result elements in the registers of a thread.  E may be A. */
#define CYB_EXPM_SMALL_MAX_N_F64 96
#define CYB_EXPM_SMALL_MAX_N_C128 64
typedef struct {
    const double* A; int64_t lda;
    int64_t n;
    int32_t a_is_real;
    int32_t reserved;
    double* E; int64_t lde;
} cyb_expm_desc;
int cyb_expm_small_batched_f64(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double alpha);
int cyb_expm_small_batched_c128(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double alpha_re, double alpha_im);
/* result_dev[i] = max_j sum_i |a_ij| of matrix i (A, lda, n, a_is_real of the descriptor; E is ignored; 0 for A == NULL or
 * n == 0): ONE launch for the list, no host synchronisation -- the norm table from which the host chooses the scaling of the
 * blocks beyond the limits above.  Column sums are added in a fixed order; the maximum is order independent. */
int cyb_norm1_batched_f64(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double* result_dev);
int cyb_norm1_batched_c128(cyb_ctx_t ctx, const cyb_expm_desc* descs, int64_t n, double* result_dev);

/* ---- grouped tensor product of blocks --------------------------------------------------------------------------------
 * Every result block of AbelianBackend::outer (src/backends/abelian.cpp:2794-2850) in ONE launch: replaces the call of
 * BlockBackend::tensor_outer (src/block_backend/block_backend.cpp:994-1010: outer + permute_axes, the result a
 * non-contiguous view) per pair of blocks (abelian.cpp:2843-2848); with k = n_a it is the plain outer of
 * _compose_no_contraction (abelian.cpp:1518-1565).
 *   dst[i_0 .. i_{k-1}, j_0 .. j_{n_b-1}, i_k .. i_{n_a-1}] = a[i_0 .. i_{n_a-1}] * b[j_0 .. j_{n_b-1}]
 * dst is C-contiguous in this axis order; a and b are read in place as strided views (strides in elements of their own
 * type).  n_a + n_b <= CYB_MAX_NDIM, 0 <= k <= n_a; entries of the shape / stride arrays beyond n_a / n_b are ignored.
 * A record with a zero extent is skipped; an empty list is valid.  Every element is one product written by one plain
 * vector store: no atomics, no zero fill, no second pass, bit-identical from run to run.  The host merges adjacent
 * axes, cuts the records into work items of bounded size and hands the kernel precomputed index increments
 * (csrc/outer_grouped.hip).  f64 entry: dst, a, b are float64 (8-byte aligned).  c128 entry: dst is interleaved
 * (re, im), 16-byte aligned; a_is_real / b_is_real != 0 say that the operand addresses float64 data (strides in doubles),
 * so that a real operand next to a complex one needs no promotion pass; a complex operand is 16-byte aligned.  The f64
 * entry ignores the two flags. */
typedef struct {
    void* dst;
    const void* a;
    const void* b;
    int32_t n_a, n_b, k;
    int32_t a_is_real, b_is_real;
    int32_t reserved;
    int64_t a_shape[CYB_MAX_NDIM];
    int64_t a_strides[CYB_MAX_NDIM];
    int64_t b_shape[CYB_MAX_NDIM];
    int64_t b_strides[CYB_MAX_NDIM];
} cyb_outer_rec;
int cyb_outer_grouped_f64(cyb_ctx_t ctx, const cyb_outer_rec* recs, int64_t n);
int cyb_outer_grouped_c128(cyb_ctx_t ctx, const cyb_outer_rec* recs, int64_t n);

/* ---- axis operations on the tree blocks of fusion-tree tensors ---------------------------------------------------------
 * FusionTreeBackend::scale_axis (src/backends/fusion_tree_backend.cpp:3521-3644) and FusionTreeBackend::_mask_contract
 * (:2372-2500) in ONE launch per tensor operation: replaces, per forest block, get_item + reshape + BlockBackend::scale_axis
 * (numpy.cpp:1373-1385) / apply_mask (:605-613) / enlarge_leg (:700-728) + reshape + set_item (:3611-3639, :2453-2494).
 * A record is one tree block of one coupled block on one side.  With the tree position t = (o * A + a) * inner + i
 * (o < outer, i < inner) counted from the start of the tree block and x < X the other matrix index, element (t, x) of the
 * source is at src + (src_start + t) * src_ts + x * src_xs, of the destination at dst + (dst_start + t') * dst_ts + x * dst_xs
 * (strides in elements of the operand's own type; a codomain record has ts = row stride, a domain record ts = column
 * stride; every block keeps its own leading dimension).
 *   CYB_TREE_SCALE   A_dst = A, dst(t, x) = table[a] * src(t, x); table: A float64 factors, or A interleaved complex ones
 *                    with table_is_complex (c128 entry only)
 *   CYB_TREE_GATHER  A_dst <= A, dst((o * A_dst + a') * inner + i, x) = src((o * A + table[a']) * inner + i, x)
 *   CYB_TREE_SCATTER A <= A_dst, dst((o * A_dst + table[a]) * inner + i, x) = src((o * A + a) * inner + i, x)
 * table of gather / scatter: int64 positions in DEVICE memory (A_dst resp. A entries, each below A resp. A_dst).
 * `fills`: regions of device memory that are set to zero before the launch (the result blocks of a scatter, and of a scale
 * whose diagonal lacks sectors: once per result block, not per record).  f64 entry: src, dst float64.  c128 entry: dst
 * interleaved (re, im), 16-byte aligned; src complex, or float64 with src_is_real (read in place, widened in the kernel).
 * Every record is validated before anything is enqueued (CYB_ERR_INVALID: negative extent, A_dst > A in a gather, NULL
 * pointer with a non-zero size, misaligned pointer).  Records with a zero extent are skipped; an empty list is valid.
 * Records of one call must not write overlapping elements. */
enum { CYB_TREE_SCALE = 0, CYB_TREE_GATHER = 1, CYB_TREE_SCATTER = 2 };
typedef struct {
    const void* src;
    void* dst;
    const void* table;
    int64_t src_ts, src_xs, dst_ts, dst_xs;
    int64_t src_start, dst_start;
    int64_t X;
    int64_t outer, A, A_dst, inner;
    int32_t mode;
    int32_t src_is_real, table_is_complex;
    int32_t reserved;
} cyb_tree_axis_rec;
typedef struct {
    void* ptr;
    int64_t bytes;
} cyb_tree_fill;
int cyb_tree_axis_f64(cyb_ctx_t ctx, const cyb_tree_axis_rec* recs, int64_t n, const cyb_tree_fill* fills, int64_t n_fills);
int cyb_tree_axis_c128(cyb_ctx_t ctx, const cyb_tree_axis_rec* recs, int64_t n, const cyb_tree_fill* fills, int64_t n_fills);

/* result_dev[0] = sum_n w_n sum_{r, c} x_n[r * x_rs + c * x_cs] * y_n[r * y_rs + c * y_cs] over a list of rows x cols views
 * (strides in elements; y == NULL: x itself, the weighted square norm).  The weights travel in the descriptors, the result
 * stays on the device, no host synchronisation.  Two stages in a fixed order, no floating-point atomics: bit-identical from
 * run to run.  Replaces the loop over coupled sectors of FusionTreeBackend::inner (fusion_tree_backend.cpp:1238-1259:
 * BlockBackend::inner per block, do_dagger = false is y read with swapped strides), ::norm (:1280-1296: BlockBackend::norm per
 * block) and ::trace_full (:1261-1278: BlockBackend::trace_full per block -- here rows = n, cols = 1, x_rs = ld + 1 and y a
 * constant one with strides 0), each of which is a reduction and a host wait per block.  c128 entry: x, y interleaved
 * complex, 16-byte aligned, result_dev[0] / [1] = (re, im); conj_x != 0 conjugates x. */
typedef struct {
    const double* x;
    const double* y;
    int64_t rows, cols;
    int64_t x_rs, x_cs, y_rs, y_cs;
    double w;
} cyb_wdot_desc;
int cyb_dot_weighted_f64(cyb_ctx_t ctx, const cyb_wdot_desc* descs, int64_t n, double* result_dev);
int cyb_dot_weighted_c128(cyb_ctx_t ctx, const cyb_wdot_desc* descs, int64_t n, int32_t conj_x, double* result_dev);

/* ---- truncation of singular values on the device -----------------------------------------
 * TensorBackend::_truncate_singular_values_selection (src/backends/tensor_backend.cpp:139-242) applied to the
 * concatenation of the per-sector singular values WITHOUT the host round trip of
 * AbelianBackend::truncate_singular_values (src/backends/abelian.cpp:3623-3638, to_numpy of all S at :3631).
 * descs[s].x / .n: the singular values of sector s (device, contiguous; at most 65536 values in total, else
 * CYB_ERR_UNSUPPORTED; up to 8192 the sort runs entirely in LDS).  Outputs (device): keep_idx_dev[off_s + j] = ascending positions (within sector s) of the kept
 * values, off_s = sum of the n of the sectors before s -- the index tables of cyb_mask_gather_batched_f64;
 * mask_dev[off_s + i] = 1 if value i of sector s is kept; result_dev[0] = err (sum of the discarded S^2),
 * result_dev[1] = new_norm (sum of the kept S^2), result_dev[2 + s] = kept count of sector s as an int64 bit pattern. */
typedef struct {
    int64_t chi_max;        /* keep at most chi_max values; < 0: no limit */
    int64_t chi_min;        /* keep at least chi_min values (>= 1) */
    double degeneracy_tol;  /* do not cut between values with log(S[i]/S[i-1]) < degeneracy_tol; 0: off */
    double trunc_cut;       /* discard while the discarded weight stays <= trunc_cut^2 */
    double svd_min;         /* keep only S >= svd_min (if has_svd_min) */
    int32_t has_svd_min;
    int32_t minimize_error; /* 1: smallest admissible cut (reference default), 0: largest */
} cyb_trunc_opts;
int cyb_truncate_select_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n_sectors, const cyb_trunc_opts* opts,
                            int64_t* keep_idx_dev, uint8_t* mask_dev, double* result_dev);
/* The same with the marginal error of a value weighted by the quantum dimension of its sector, err_i = d_s * S_i^2 -- the
 * `qdims` argument of tensor_backend.cpp:158-164, which FusionTreeBackend::truncate_singular_values fills with ONE number
 * per coupled sector (fusion_tree_backend.cpp:2280-2303).  sector_weights: n_sectors positive numbers on the HOST, or NULL
 * (all 1: the abelian case).  err and new_norm are the weighted sums. */
int cyb_truncate_select_weighted_f64(cyb_ctx_t ctx, const cyb_vec_desc* descs, int64_t n_sectors, const double* sector_weights,
                                     const cyb_trunc_opts* opts, int64_t* keep_idx_dev, uint8_t* mask_dev, double* result_dev);

/* ---- segment ops: arithmetic, reductions and compaction of lists of 1-D sector blocks ---------------------------------
 * What a tensor-network code does with a DiagonalTensor (singular values) or a Mask after a decomposition, for ALL sectors
 * in ONE launch per call (csrc/segment_ops.hip).  A *segment* is one contiguous 1-D sector block; a record names up to
 * two operand segments and an output of the same length n.  Operand kinds: CYB_SEG_ABSENT (read as zeros: a sector
 * without a block, no zero block is allocated), CYB_SEG_F64, CYB_SEG_C128 (interleaved) and CYB_SEG_BOOL (one byte per
 * element).  Pointers are aligned to 8 bytes (numeric kinds); 16-byte accesses are used where a pointer allows them.
 * n == 0, n == 1 and an empty list are valid.  All three entries are bit-identical from run to run and a segment's result
 * depends on nothing but the segment: the owner of a segment (16 lanes for n <= 64, one wave for n <= 1024, one
 * workgroup for n <= 16384, one workgroup per 16384-element chunk above) and the combination order are fixed by n alone; no
 * float atomics (an integer ticket elects the workgroup that adds the chunk partials in chunk order).
 *
 * cyb_seg_binary: out = a (op) b elementwise.  Replaces the per-sector func(block_a, block_b) of
 * AbelianBackend::diagonal_elementwise_binary (src/backends/abelian.cpp:1596-1619) and of mask_binary_operand /
 * mask_unary_operand (:2410-2427, :2705-2714), and the zero blocks they allocate for missing sectors (:1605, :1615, :2417,
 * :2425, :2712).  Arithmetic ops write out_kind F64 or C128 (a real operand next to a complex one is read in place);
 * comparisons and logical ops write BOOL.  With use_scalar != 0 operand b of EVERY record is the scalar (re, im).  The
 * ordering comparisons use the real parts (callers reject complex operands); logical ops read "non-zero" as true, NOT
 * ignores b.
 *
 * cyb_seg_reduce: one number per segment (operand a; b and out are ignored), result_dev[2 s] / [2 s + 1] = (re, im) or
 * (value, 0).  Replaces block_func(block) per sector of reduce_DiagonalTensor (:3163-3173), sum_all per sector of
 * diagonal_tensor_trace_full (:970-971) and all / any per sector of diagonal_all / diagonal_any (:726-738), each of them a
 * launch and a host synchronisation.  The pre-map is applied to every element on the fly (real segments; ABS also takes
 * complex ones).  An absent segment is reduced as n zeros; n == 0 gives 0 (SUM, COUNT), -inf (MAX), +inf (MIN).  MAX / MIN
 * compare real parts and skip NaN (fmax / fmin).
 *
 * cyb_seg_compact: per segment (operand a: the flags, BOOL or numeric with non-zero = keep) the ascending kept positions
 * keep_idx_dev[off_s + j], off_s = sum of the n of the segments before s, and counts_dev[s] = number kept -- the table
 * layout of cyb_truncate_select_f64, read by cyb_mask_gather_batched_f64 / cyb_mask_scatter_batched_f64.  Replaces any /
 * sum_all / to_numpy per sector of diagonal_to_mask (:1707-1728) and sum_all per sector of mask_binary_operand (:2428) and
 * mask_unary_operand (:2715).  A workgroup that owns a later chunk of a long segment recounts the flags before its chunk
 * (quadratic in the number of chunks; bond dimensions stay far below that mattering). */
#define CYB_SEG_ABSENT 0
#define CYB_SEG_F64 1
#define CYB_SEG_C128 2
#define CYB_SEG_BOOL 3
enum { CYB_SEG_ADD = 0, CYB_SEG_SUB, CYB_SEG_MUL, CYB_SEG_DIV, CYB_SEG_LT, CYB_SEG_LE, CYB_SEG_GT, CYB_SEG_GE, CYB_SEG_EQ,
       CYB_SEG_NE, CYB_SEG_AND, CYB_SEG_OR, CYB_SEG_XOR, CYB_SEG_NOT, CYB_SEG_N_OPS };
enum { CYB_SEG_SUM = 0, CYB_SEG_MAX, CYB_SEG_MIN, CYB_SEG_COUNT, CYB_SEG_N_REDUCE };
enum { CYB_SEG_PRE_NONE = 0, CYB_SEG_PRE_ABS, CYB_SEG_PRE_SQUARE, CYB_SEG_PRE_XLOGX /* x log x for x > param, else 0 */,
       CYB_SEG_PRE_POW /* x^param */, CYB_SEG_N_PRE };
typedef struct {
    const void* a;
    const void* b;
    void* out;
    int64_t n;
    int32_t a_kind, b_kind, out_kind;
    int32_t reserved;
} cyb_seg_rec;
int cyb_seg_binary(cyb_ctx_t ctx, const cyb_seg_rec* recs, int64_t n_segs, int32_t op, int32_t use_scalar, double scalar_re,
                   double scalar_im);
int cyb_seg_reduce(cyb_ctx_t ctx, const cyb_seg_rec* recs, int64_t n_segs, int32_t op, int32_t pre, double param,
                   double* result_dev);
int cyb_seg_compact(cyb_ctx_t ctx, const cyb_seg_rec* recs, int64_t n_segs, int64_t* keep_idx_dev, int64_t* counts_dev);

/* fill: out[i] = value (zeros / ones_block); eye: out (n x n, contiguous) = identity
 * (eye_matrix, numpy.cpp:1197-1207) */
int cyb_fill_f64(cyb_ctx_t ctx, double* out, int64_t n, double value);
int cyb_eye_f64(cyb_ctx_t ctx, double* out, int64_t n);
/* counter-based standard-normal fill (random_normal; Philox4x32-10 + Box-Muller), sigma-scaled */
int cyb_random_normal_f64(cyb_ctx_t ctx, double* out, int64_t n, uint64_t seed, double sigma);
/* counter-based uniform fill on [lo, hi) (random_uniform, numpy.cpp:965-988 draws from [-1, 1)) */
int cyb_random_uniform_f64(cyb_ctx_t ctx, double* out, int64_t n, uint64_t seed, double lo, double hi);

#ifdef __cplusplus
}
#endif
#endif /* CYTEN_AMD_H */
