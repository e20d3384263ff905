"""Host side of the batched decompositions -- SVD, QR / LQ, eigh -- of `HipBlockBackend`.

Plain functions that take the backend first: `HipBlockBackend` binds them as its methods, and everything in here calls back
through the backend's methods (`bb.matrix_qr_batched`, `bb.matrix_dot_grouped`, `bb.lincomb_many`, ...).  Which route a
block takes and which check it gets is stated once per kind: `matrix_svd_batched`, `matrix_qr_batched`, `eigh_batched`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

# ---- thresholds of the embedded complex routes (the `*_EMBED_*` ones are also attributes of `HipBlockBackend`: the routes read them there)
# complex blocks with min(m, n) at least this large are decomposed on the float64 block engine through the embedding
# (measured: 96 -> 4.7 vs 4.7 ms, 192 -> 10.0 vs 11.3 ms, 1024 -> 111 vs 220 ms, sixteen 128-blocks -> 13.7 vs 21.3 ms)
COMPLEX_SVD_EMBED_MIN = 96
# complex blocks with min(m, n) at least this large take the embedded route of `complex_qr_embedded`
COMPLEX_QR_EMBED_MIN = 48
# ... up to this many rows (the embedding has twice as many; beyond 1536 real rows the blocked QR spreads a panel over
# several workgroups, qr_panel_multi_kernel, which must all be resident: 256 CUs x 1536 rows)
COMPLEX_QR_EMBED_MAX_ROWS = 65536
# ... and so do smaller ones with max(m, n) beyond this, the largest extent of the one-workgroup kernel of csrc/cqr_house.hip
COMPLEX_QR_ONE_WORKGROUP_MAX = 128
# complex Hermitian blocks at least this large are diagonalised on the float64 block engine through the embedding
# (measured: 128 -> 4.5 vs 5.5 ms, 448 -> 24 vs 40 ms, 1024 -> 85 vs 181 ms, sixteen 256-blocks -> 13 vs 68 ms; the in-LDS
#  kernel of csvd_small.hip serves n <= 64 in 1.6 ms)
COMPLEX_EIGH_EMBED_MIN = 96
# ---- tolerances of the checks behind the embedded routes
# defect |U^H U - 1| above which a factor of the embedded route is re-orthonormalised: half of the 1e-13 that
# tests/test_gpu_decomp_accuracy.py holds every factor to.  Full-rank, mildly graded blocks come out at 1e-14 ... 3e-13 --
# an eightfold degenerate 128 x 128 block at 1.4e-13 (U) and, with the LQ step, 3.7e-13 (Vh), which the earlier 2e-12 let
# through; the complex QR behind the check leaves 1e-14
COMPLEX_SVD_ORTHO_TOL = 5e-14
# |U S Vh - A|_max above this (times sqrt(max(m, n)) max|A|) sends a block of the embedded route to the complex kernels
# (structured blocks come out at 1e-15 ... 1e-14 on this scale)
COMPLEX_SVD_RECON_TOL = 1e-12
# unitarity defect |Q^H Q - 1| above which the factor of the embedded QR is re-orthonormalised
COMPLEX_QR_ORTHO_TOL = 1e-12
# ... and above which, after that second pass, the block is handed back to the complex Householder kernels
COMPLEX_QR_SECOND_PASS_TOL = 1e-11
# |Q R - A|_max above this (times max(m, n) max|A|) hands a block of the embedded QR back as well
COMPLEX_QR_RECON_TOL = 1e-11


# ---- shared pieces
def _sources(bb, blocks):
    """(contiguous sources, complex?): one complex block makes the whole list complex."""
    bb._numeric_only(blocks, 'decomposition')
    cplx = any(b.is_complex for b in blocks)
    if cplx:
        blocks = [bb.as_complex(b) for b in blocks]
    return bb.contiguous_many(blocks), cplx


def _route(srcs, big, embedded, direct):
    """Per-block results of a complex list: `embedded` on the blocks `big`, `direct` -- one call -- on all others and on
    the blocks `embedded` hands back (None in its list), merged by index.  None if `big` is empty (as for every float64
    list) or `embedded` refuses its list as a whole (returns None): the caller then takes the direct route for all of it."""
    got = embedded([srcs[i] for i in big]) if big else None
    if got is None:
        return None
    done = {i: g for i, g in zip(big, got) if g is not None}
    rest = [i for i in range(len(srcs)) if i not in done]
    done.update(zip(rest, direct([srcs[i] for i in rest]) if rest else []))
    return [done[i] for i in range(len(srcs))]


def _per_block(got):
    """(results, info, ...) of a list -> one tuple per block; None (the list was refused) stays None."""
    return None if got is None else list(zip(*got))


def _view(bb, blk, offset, shape, strides):
    """A strided view into the buffer of `blk`, `offset` elements behind its first one."""
    return type(blk)(bb, blk.buf, blk.offset + offset, shape, strides)


def _products(bb, lefts, rights):
    """left_i @ right_i for the whole list: ONE grouped GEMM."""
    return bb.matrix_dot_grouped([[(l, r)] for l, r in zip(lefts, rights)])


def _gram_defect(bb, gram, eyes):
    """G - 1 for one Gram matrix; `eyes` caches the identity per size."""
    k = gram.shape[0]
    if k not in eyes:
        eyes[k] = bb.eye_matrix(k, dtype='complex128')
    return bb.linear_combination(1.0, gram, -1.0, eyes[k])


def embed_complex(bb, srcs):
    """Interleaved real embeddings M(A) (a + ib -> [[a, -b], [b, a]]; 2m x 2n float64) of contiguous complex 2-D blocks:
    one buffer, ONE strided launch."""
    Ms = bb._new_many([(2 * a.shape[0], 2 * a.shape[1]) for a in srcs])
    items = []
    for a, M in zip(srcs, Ms):
        m, nn = a.shape
        if m * nn == 0:
            continue
        re, im = bb._plane(a, 0), bb._plane(a, 1)
        for off, coeff, src in ((0, 1.0, re), (1, -1.0, im), (2 * nn, 1.0, im), (2 * nn + 1, 1.0, re)):
            items.append((_view(bb, M, off, (m, nn), (4 * nn, 2)), [(coeff, src)], False))
    bb.lincomb_many(items)
    return Ms


def extract_complex_items(bb, X, out, by_rows=False):
    """lincomb items that read the complex matrix out of a structured embedding X into the complex block `out` (r x c):
    from the even COLUMNS of X (real part rows 0::2, imaginary part rows 1::2 -- a real column of X is one complex
    column), or with `by_rows` from the even ROWS (real part columns 0::2, imaginary part minus columns 1::2 -- a
    real row of X is one complex row)."""
    r, c = out.shape
    if r * c == 0:
        return []
    ld = X.strides[0]
    fo = bb._fview(out)
    return [(_view(bb, fo, plane, (r, c), (2 * c, 2)), [(coeff, _view(bb, X, off, (r, c), (2 * ld, 2)))], False)
            for plane, off, coeff in (((0, 0, 1.0), (1, 1, -1.0)) if by_rows else ((0, 0, 1.0), (1, ld, 1.0)))]


# ---- SVD
def _svd_outs(bb, srcs, cplx, given=None):
    """[(U, S, Vh)] for 2-D sources: float64 triples out of one buffer, or complex U / Vh out of one and float64 S out of
    another, or the caller's `given` triples once they are found to fit."""
    kshapes = [(a.shape[0], min(a.shape), a.shape[1]) for a in srcs]
    if given is not None:
        for (m, k, nn), (U, S, Vh) in zip(kshapes, given):
            if U.shape != (m, k) or S.shape != (k,) or Vh.shape != (k, nn) or not (
                    U.is_contiguous() and S.is_contiguous() and Vh.is_contiguous()):
                raise ValueError('matrix_svd_batched: outs[i] must be contiguous (m,k), (k,), (k,n) blocks')
        return [tuple(o) for o in given][:len(srcs)]
    if cplx:
        cflat = bb._new_many([sh for m, k, nn in kshapes for sh in ((m, k), (k, nn))], True)
        rflat = bb._new_many([(k,) for _, k, _ in kshapes])
        return [(cflat[2 * i], rflat[i], cflat[2 * i + 1]) for i in range(len(srcs))]
    flat = bb._new_many([sh for m, k, nn in kshapes for sh in ((m, k), (k,), (k, nn))])
    return [tuple(flat[3 * i:3 * i + 3]) for i in range(len(srcs))]


def _svd_launch(bb, srcs, outs, cplx, return_info, null_vectors=True, return_rank=False, embedded=False):
    """One C-ABI call for contiguous 2-D sources (`embedded`: embeddings of complex blocks): `cyb_svd_batched_c128` for complex
    blocks, `cyb_svd_batched_f64` for float64 blocks with null vectors and without ranks, else `cyb_svd_batched_ex_f64` (null
    vectors skipped and / or ranks reported; the embedded route).  Returns (status, info, ranks); the caller checks the status."""
    n = len(srcs)
    if not n:
        return _lib.CYB_OK, [], []
    arr = np.zeros(n, dtype=_lib.SVD_DTYPE)
    ms, ns = np.array([a.shape for a in srcs], dtype=np.int64).T
    arr['A'], arr['m'], arr['n'] = [a.ptr for a in srcs], ms, ns
    arr['lda'] = arr['ldvh'] = np.maximum(ns, 1)
    arr['ldu'] = np.maximum(np.minimum(ms, ns), 1)
    arr['U'], arr['S'], arr['Vh'] = [o[0].ptr for o in outs], [o[1].ptr for o in outs], [o[2].ptr for o in outs]
    descs = arr.ctypes.data_as(C.POINTER(_lib.SvdDesc))
    info, rank = (C.c_int32 * n)(), (C.c_int32 * n)()
    pinfo = info if return_info or embedded else None
    bb.ctx.sync_stream()
    if cplx or (null_vectors and not return_rank and not embedded):
        st = (bb.lib.cyb_svd_batched_c128 if cplx else bb.lib.cyb_svd_batched_f64)(bb.ctx.handle, descs, n, pinfo)
        rank[:] = [min(a.shape) for a in srcs]
    else:
        flags = (_lib.CYB_SVD_EMBEDDED_COMPLEX if embedded else 0) | (0 if null_vectors else _lib.CYB_SVD_SKIP_NULL_VECTORS)
        st = bb.lib.cyb_svd_batched_ex_f64(bb.ctx.handle, descs, n, pinfo, flags, rank)
    return st, list(info), list(rank)


def _svd_direct(bb, srcs, cplx, given, return_info, null_vectors=True, return_rank=False):
    outs = _svd_outs(bb, srcs, cplx, given)
    st, info, rank = _svd_launch(bb, srcs, outs, cplx, return_info, null_vectors, return_rank)
    _lib.check(st)
    return outs, info, rank


def svd_complex_direct(bb, srcs, return_info=False):
    """The complex Jacobi kernels (`cyb_svd_batched_c128`) on contiguous complex 2-D blocks, without the embedded route."""
    outs, info, _ = _svd_direct(bb, srcs, True, None, return_info)
    return (outs, info) if return_info else outs


def matrix_svd_batched(bb, blocks, algorithm=None, return_info=False, outs=None, null_vectors=True, return_rank=False):
    """Thin SVD of every 2-D block of a list in one batched call.  Returns [(U, S, Vh)], S descending
    (scipy.linalg.svd(full_matrices=False) conventions, numpy.cpp:1247-1297).  All reference algorithm names are accepted
    and map to the block-Jacobi kernel.
    Routes.  float64 lists: `cyb_svd_batched_f64`, or `cyb_svd_batched_ex_f64` when null vectors are skipped or ranks are
    wanted (the truncating caller's form).  Complex lists: blocks with min(m, n) >= `COMPLEX_SVD_EMBED_MIN` take
    `complex_svd_embedded`, which serves that form too and checks what it returns; the others -- and the whole list if the
    engine refuses it -- take the complex Jacobi kernels (`svd_complex_direct`), which always complete and report k."""
    if algorithm is not None and algorithm not in bb.svd_algorithms:
        raise ValueError(f'SVD algorithm not supported: {algorithm}')
    if outs is not None and any(b.is_complex for b in blocks):
        raise NotImplementedError('matrix_svd_batched: preallocated outputs are for float64 blocks')
    srcs, cplx = _sources(bb, blocks)
    if any(a.ndim != 2 for a in srcs):
        raise ValueError('matrix_svd: block must be 2-D')
    routed = _route(srcs, [i for i, a in enumerate(srcs) if cplx and min(a.shape) >= bb.COMPLEX_SVD_EMBED_MIN],
                    lambda big: _per_block(bb._complex_svd_embedded(big, True, null_vectors)),
                    lambda rest: [(r, f, min(a.shape)) for a, r, f in zip(rest, *bb.matrix_svd_batched_complex_direct(rest, True))])
    res, info, rank = zip(*routed) if routed is not None else _svd_direct(bb, srcs, cplx, outs, return_info, null_vectors, return_rank)
    out = (list(res),) + ((list(info),) if return_info else ()) + ((list(rank),) if return_rank else ())
    return out if len(out) > 1 else out[0]


def complex_svd_embedded(bb, srcs, return_info=False, null_vectors=True):
    """Thin SVD of complex blocks on the float64 block engine: the pipeline of the real SVD --
    blocked QR, LQ step, persistent block-Jacobi sweeps, completion from Q2 -- runs on the interleaved embeddings
    with `CYB_SVD_EMBEDDED_COMPLEX`: its QR steps preserve the structure by uniqueness, its pivot solves by
    construction (a complex 16 x 16 Hermitian Jacobi solve per pair), rows are deflated / ranked / completed as
    pairs.  Returns ([(U, S, Vh)], info, ranks) in complex / float64 blocks (ranks: numerical ranks in complex rows;
    with `null_vectors=False` the vectors beyond a block's rank are unspecified, CYB_SVD_SKIP_NULL_VECTORS), or None
    if the engine refuses the list: the caller then uses the complex Jacobi kernels.
    Checks: a factor whose |U^H U - 1| or |Vh Vh^H - 1| exceeds `COMPLEX_SVD_ORTHO_TOL` is re-orthonormalised by a complex
    QR; a block whose |U S Vh - A| then misses `COMPLEX_SVD_RECON_TOL` is decomposed again by the complex Jacobi kernels."""
    n = len(srcs)
    Ms = embed_complex(bb, srcs)
    real = _svd_outs(bb, Ms, False)
    st, info, rank = _svd_launch(bb, Ms, real, False, True, null_vectors, embedded=True)
    if st == _lib.CYB_ERR_UNSUPPORTED:
        return None
    if st != _lib.CYB_ERR_NOCONV:   # (blocks that did not settle are caught by the reconstruction check below)
        _lib.check(st)
    res = _svd_outs(bb, srcs, True)
    # real column 2a of U and real row 2a of Vh are ONE real singular triplet: a complex triplet whatever the
    # basis the engine left inside the two-dimensional real singular subspace
    bb.lincomb_many([it for (U, _, Vh), (Uc, _, Vhc) in zip(real, res)
                     for it in extract_complex_items(bb, U, Uc) + extract_complex_items(bb, Vh, Vhc, by_rows=True)])
    bb.copy_many([(Sc, _view(bb, S, 0, Sc.shape, (2,))) for (_, S, _), (_, Sc, _) in zip(real, res)])
    cranks = [int(r) // 2 for r in rank]
    # (columns that count: all of them, or -- null vectors skipped -- the leading rank)
    kk = [min(srcs[i].shape) if null_vectors else cranks[i] for i in range(n)]
    # (info < 0 with rank 0: a block the engine left out because it holds NaN or Inf -- nothing was written for it, the
    #  complex Jacobi kernels below get it and report the failure)
    left_out = [i for i in range(n) if info[i] < 0 and int(rank[i]) == 0 and min(srcs[i].shape) > 0]
    todo = [i for i in range(n) if kk[i] > 0 and i not in left_out]

    def redo(failing):
        fres, finfo = bb.matrix_svd_batched_complex_direct([srcs[i] for i in failing], True)
        for i, r, f in zip(failing, fres, finfo):
            res[i], info[i], cranks[i] = r, f, min(srcs[i].shape)
        return res, info, cranks

    if not todo:
        if left_out:
            return redo(left_out)
        _lib.check(st)   # (no convergence, and no block to check)
        return res, info, cranks
    # Orthonormality in the COMPLEX sense ("Read-off"): the even real columns of U (rows of Vh) are
    # orthonormal as real vectors; as complex vectors only as far as Q1's reflectors are structured, and those built from a
    # trailing block near the rounding level of the matrix are not (defect eps * sigma_max / sigma_j).  One grouped GEMM
    # measures the defect; where it shows, a complex QR of the factor (columns in order of descending sigma) restores it.
    us = [bb.subblock(res[i][0], 0, srcs[i].shape[0], 0, kk[i]) for i in todo]
    vs = [bb.subblock(res[i][2], 0, kk[i], 0, srcs[i].shape[1]) for i in todo]
    uh = [bb.dagger(u) for u in us]
    vt = [bb.dagger(v) for v in vs]
    uc = bb.contiguous_many(us)
    grams = _products(bb, uh + vs, uc + vt)
    eyes = {}
    bad_u, bad_v = [], []
    for j in range(len(todo)):
        for g, lst in ((grams[j], bad_u), (grams[len(todo) + j], bad_v)):
            if not bb.max_abs(_gram_defect(bb, g, eyes)) <= COMPLEX_SVD_ORTHO_TOL:
                lst.append(j)
    if bad_u or bad_v:
        qs = [q for q, _ in bb.matrix_qr_batched([uc[j] for j in bad_u] + [vt[j] for j in bad_v], False)]
        bb.copy_many([(us[j], qs[t]) for t, j in enumerate(bad_u)])
        bb.copy_many([(vs[j], bb.permute_axes(qs[len(bad_u) + t], [1, 0])) for t, j in enumerate(bad_v)], conj=True)
    # Reconstruction check.  The route rests on the QR steps leaving R = M(R_c) structured, which needs the leading
    # columns of the block to be independent: a numerically dependent column in the MIDDLE (zero columns, a product of
    # block-sparse factors) gets an unstructured reflector pair and the rows of R after it are no partners any more
    # (singular values off by 1e-3, or no convergence; scripts/svd_fuzz.py seeds 52 / 53).  One grouped GEMM per list
    # finds those blocks; they go to the complex Jacobi kernels, which make no such assumption.
    ss = [_view(bb, res[i][1], 0, (kk[i],), (1,)) for i in todo]
    recon = _products(bb, bb.scale_axis_many([(u, sv, 1) for u, sv in zip(us, ss)]), vs)
    diffs = bb.linear_combination_many(1.0, recon, -1.0, [srcs[i] for i in todo])
    failing = [i for j, i in enumerate(todo)
               if not bb.max_abs(diffs[j]) <= COMPLEX_SVD_RECON_TOL * np.sqrt(max(srcs[i].shape)) * bb.max_abs(srcs[i])]
    failing = sorted(failing + left_out)
    return redo(failing) if failing else (res, info, cranks)


# ---- QR / LQ
def _qr_outs(bb, srcs, full, cplx):
    """[(Q, R)] of one dtype for 2-D sources, out of one buffer."""
    if any(a.ndim != 2 for a in srcs):
        raise ValueError('matrix_qr: block must be 2-D')
    kshapes = [(a.shape[0], a.shape[0] if full else min(a.shape), a.shape[1]) for a in srcs]
    flat = bb._new_many([sh for m, kq, nn in kshapes for sh in ((m, kq), (kq, nn))], cplx)
    return [tuple(flat[2 * i:2 * i + 2]) for i in range(len(srcs))]


def _qr_launch(bb, srcs, outs, full, cplx):
    """One C-ABI call for contiguous 2-D sources of one dtype: `cyb_qr_batched_c128` or `cyb_qr_batched_f64`."""
    n = len(srcs)
    if not n:
        return _lib.CYB_OK
    arr = np.zeros(n, dtype=_lib.QR_DTYPE)
    ms, ns = np.array([a.shape for a in srcs], dtype=np.int64).T
    arr['A'], arr['m'], arr['n'] = [a.ptr for a in srcs], ms, ns
    arr['lda'] = arr['ldr'] = np.maximum(ns, 1)
    arr['ldq'] = np.maximum(ms if full else np.minimum(ms, ns), 1)
    arr['Q'], arr['R'] = [o[0].ptr for o in outs], [o[1].ptr for o in outs]
    arr['full'] = int(full)
    bb.ctx.sync_stream()
    fn = bb.lib.cyb_qr_batched_c128 if cplx else bb.lib.cyb_qr_batched_f64
    return fn(bb.ctx.handle, arr.ctypes.data_as(C.POINTER(_lib.QrDesc)), n)


def qr_direct(bb, srcs, full, cplx):
    """The QR kernels of the C-ABI on contiguous 2-D blocks of one dtype (`cyb_qr_batched_f64` / `_c128`), without the
    embedded route."""
    outs = _qr_outs(bb, srcs, full, cplx)
    _lib.check(_qr_launch(bb, srcs, outs, full, cplx))
    return outs


def matrix_qr_batched(bb, blocks, full=False):
    """QR of every 2-D block (scipy.linalg.qr mode 'economic'/'full', numpy.cpp:1236-1245).
    Routes.  float64 lists: the blocked Householder QR of `cyb_qr_batched_f64`.  Complex lists, economic and full: non-empty
    blocks with min(m, n) >= `COMPLEX_QR_EMBED_MIN` or max(m, n) > `COMPLEX_QR_ONE_WORKGROUP_MAX`, of up to
    `COMPLEX_QR_EMBED_MAX_ROWS` rows, take `complex_qr_embedded`, which checks unitarity and reconstruction per block; the
    blocks it gives up and all others take complex Householder QR (`cyb_qr_batched_c128`, csrc/cqr_house.hip), which is
    backward stable for every block."""
    srcs, cplx = _sources(bb, blocks)
    big = [i for i, a in enumerate(srcs) if cplx and a.ndim == 2 and min(a.shape) > 0 and a.shape[0] <= bb.COMPLEX_QR_EMBED_MAX_ROWS
           and (min(a.shape) >= bb.COMPLEX_QR_EMBED_MIN or max(a.shape) > COMPLEX_QR_ONE_WORKGROUP_MAX)]
    routed = _route(srcs, big, lambda s: bb._complex_qr_embedded(s, full), lambda s: bb.matrix_qr_batched_direct(s, full, True))
    return routed if routed is not None else bb.matrix_qr_batched_direct(srcs, full, cplx)


def complex_qr_embedded(bb, srcs, full=False, _depth=0):
    """QR of complex blocks on the real block engine: the REAL blocked Householder QR of the
    interleaved embedding M(A) -- entry a + ib -> [[a, -b], [b, a]], 2m x 2n -- IS the complex QR once the diagonal of
    R is made positive (a QR with fixed diagonal signs is unique, and M(R_c) is upper triangular in the interleaved
    column order), so the MFMA strip kernel and the register-resident panel kernels serve complex blocks unchanged.
    Q_c is the even real columns of Q (real column 2a IS complex column a), R_c the even rows of R.

    That argument needs full column rank.  Where the block is numerically rank deficient -- or only has a part at the
    level eps |A| / sigma, e.g. a low-rank block plus noise -- the reflectors built from the trailing block carry no
    (or only part of the) structure: the even columns are then still orthonormal as REAL vectors and A = Q R still holds,
    but they are not orthonormal in the complex sense (defect eps |A| / sigma_j, up to O(1)).  One grouped GEMM measures
    the defect; above `COMPLEX_QR_ORTHO_TOL` the factor is factored once more, Q_c = Q' S (a well-conditioned block:
    its embedded QR is structured to rounding), and A = Q' (S R_c) with S R_c upper triangular -- "twice is enough".
    `full`: the extra m - k columns are the even columns of the real full Q's trailing part, made orthonormal with the
    rest by the same second pass.  `scripts/complex_embedding_model.py` is the numpy check of the argument.
    Returns [(Q, R)], with None for a block whose second pass is still above `COMPLEX_QR_SECOND_PASS_TOL` or whose
    |Q R - A| misses `COMPLEX_QR_RECON_TOL`: the caller factors those with the complex Householder kernels."""
    n = len(srcs)
    qrs = bb.matrix_qr_batched(embed_complex(bb, srcs), full)
    # diagonal of every R to the host: signs for the uniqueness fix
    diags = [bb.contiguous(_view(bb, R, 0, (min(R.shape),), (R.strides[0] + 1,))) if min(R.shape) else None for _, R in qrs]
    fix_q, fix_r = [], []
    for (Q, R), d in zip(qrs, diags):
        sq, sr = np.ones(Q.shape[1]), np.ones(R.shape[0])
        if d is not None:
            sgn = np.where(bb.to_numpy(d) < 0, -1.0, 1.0)
            sq[:len(sgn)] = sr[:len(sgn)] = sgn
        fix_q.append((Q, bb.as_block(sq), 1))
        fix_r.append((R, bb.as_block(sr), 0))
    Qs = bb.scale_axis_many(fix_q)
    Rs = bb.scale_axis_many(fix_r)
    outs = _qr_outs(bb, srcs, full, True)
    bb.lincomb_many([it for Qe, Re, (Q, R) in zip(Qs, Rs, outs)
                     for it in extract_complex_items(bb, Qe, Q) + extract_complex_items(bb, Re, R)])
    # ---- complex unitarity of the extracted factors; second pass where it is not there
    todo = [i for i in range(n) if outs[i][0].shape[1] > 0 and outs[i][0].shape[0] > 0]
    if todo and _depth < 2:
        eyes = {}
        qs = [outs[i][0] for i in todo]
        diffs = [_gram_defect(bb, g, eyes) for g in _products(bb, [bb.dagger(q) for q in qs], qs)]
        bad = []
        if not bb.max_abs_many(diffs) <= COMPLEX_QR_ORTHO_TOL:   # (one read-back for the list; per block only if needed)
            bad = [i for i, df in zip(todo, diffs) if not bb.max_abs(df) <= COMPLEX_QR_ORTHO_TOL]
        if bad:
            second = bb._complex_qr_embedded([outs[i][0] for i in bad], False, _depth + 1)
            newr = _products(bb, [S for _, S in second], [outs[i][1] for i in bad])
            for i, (Q2, _), R2 in zip(bad, second, newr):
                outs[i] = (Q2, R2)
            if _depth == 0:   # the re-factored blocks are measured once more; what is still not unitary is handed back
                qs = [outs[i][0] for i in bad]
                for i, g in zip(bad, _products(bb, [bb.dagger(q) for q in qs], qs)):
                    if not bb.max_abs(_gram_defect(bb, g, eyes)) <= COMPLEX_QR_SECOND_PASS_TOL:
                        outs[i] = None
                todo = [i for i in todo if outs[i] is not None]
    if _depth == 0 and todo:
        # The structure argument also fails when a numerically DEPENDENT column sits in the middle of the block (an
        # unstructured reflector pair there leaves a complement that is not invariant either, and every later column pair
        # inherits it): A = Q_c R_c then no longer holds.  One more grouped GEMM checks the reconstruction; such blocks go
        # back to the caller (None), which uses complex Householder QR: a dependent column there simply gets tau = 0.
        prods = _products(bb, [outs[i][0] for i in todo], [outs[i][1] for i in todo])
        for j, i in enumerate(todo):
            scale = bb.max_abs(srcs[i])
            if scale != 0.0 and not bb.max_abs(bb.linear_combination(1.0, prods[j], -1.0, srcs[i])) <= COMPLEX_QR_RECON_TOL * scale * max(srcs[i].shape):
                outs[i] = None
    return outs


def matrix_lq_batched(bb, blocks, full=False):
    """block_backend.cpp:1033-1040: q, r = qr(a^T); return r^T, q^T (views).  Routes: those of the QR of the transposes."""
    qrs = bb.matrix_qr_batched([bb.permute_axes(a, [1, 0]) for a in blocks], full)
    return [(bb.permute_axes(r, [1, 0]), bb.permute_axes(q, [1, 0])) for q, r in qrs]


# ---- eigh
def _eigh_outs(bb, srcs, vectors, cplx):
    """[(w, V)] for square sources: float64 pairs out of one buffer (V is None without `vectors`), or float64 w out of
    one buffer and complex V out of another."""
    if cplx:
        return list(zip(bb._new_many([(a.shape[0],) for a in srcs]), bb._new_many([(a.shape[0], a.shape[0]) for a in srcs], True)))
    if not vectors:
        return [(w, None) for w in bb._new_many([(a.shape[0],) for a in srcs])]
    flat = bb._new_many([sh for a in srcs for sh in ((a.shape[0],), (a.shape[0], a.shape[0]))])
    return [(flat[2 * i], flat[2 * i + 1]) for i in range(len(srcs))]


def _eigh_launch(bb, srcs, outs, cplx, return_info, embedded=False):
    """One C-ABI call for contiguous square sources: `cyb_eigh_batched_ex_f64` for the `embedded` route (embeddings of complex
    Hermitian blocks), else `cyb_eigh_batched_c128` / `cyb_eigh_batched_f64`.  Returns (status, info); the caller checks the status."""
    n = len(srcs)
    if not n:
        return _lib.CYB_OK, []
    arr = np.zeros(n, dtype=_lib.EIGH_DTYPE)
    ks = np.array([a.shape[0] for a in srcs], dtype=np.int64)
    arr['A'], arr['n'] = [a.ptr for a in srcs], ks
    arr['lda'] = arr['ldv'] = np.maximum(ks, 1)
    arr['W'] = [w.ptr for w, _ in outs]
    if outs[0][1] is not None:
        arr['V'] = [v.ptr for _, v in outs]
    descs = arr.ctypes.data_as(C.POINTER(_lib.EighDesc))
    info = (C.c_int32 * n)()
    bb.ctx.sync_stream()
    if embedded:
        st = bb.lib.cyb_eigh_batched_ex_f64(bb.ctx.handle, descs, n, info, _lib.CYB_EIGH_EMBEDDED_COMPLEX)
    else:
        fn = bb.lib.cyb_eigh_batched_c128 if cplx else bb.lib.cyb_eigh_batched_f64
        st = fn(bb.ctx.handle, descs, n, info if return_info else None)
    return st, list(info)


def eigh_direct(bb, srcs, vectors=True, return_info=False):
    """The eigh kernels of the C-ABI on contiguous square blocks of one dtype, without the embedded route: [(w ascending, V)] from
    `cyb_eigh_batched_f64` (V is None without `vectors`) or the complex Jacobi kernels of `cyb_eigh_batched_c128` (always with V)."""
    cplx = any(a.is_complex for a in srcs)
    outs = _eigh_outs(bb, srcs, vectors, cplx)
    st, info = _eigh_launch(bb, srcs, outs, cplx, return_info)
    _lib.check(st)
    return (outs, info) if return_info else outs


def eigh_batched(bb, blocks, sort=None, vectors=True, return_info=False):
    """Hermitian EVD of every block: [(w ascending, V)] (np.linalg.eigh, numpy.cpp:658-680).
    Routes.  float64 lists: `cyb_eigh_batched_f64`.  Complex lists: blocks with n >= `COMPLEX_EIGH_EMBED_MIN` take
    `complex_eigh_embedded` (no check behind it: the embedding is exactly structured); the others -- and the whole list if
    the engine refuses it -- take the complex Jacobi kernels (csrc/csvd_small.hip, csrc/csvd_large.hip)."""
    srcs, cplx = _sources(bb, blocks)
    if any(a.ndim != 2 or a.shape[0] != a.shape[1] for a in srcs):
        raise ValueError('eigh: block must be a square matrix')
    routed = _route(srcs, [i for i, a in enumerate(srcs) if cplx and a.shape[0] >= bb.COMPLEX_EIGH_EMBED_MIN],
                    lambda big: _per_block(bb._complex_eigh_embedded(big, True)),
                    lambda rest: _per_block(bb.eigh_batched_direct(rest, True, True)))
    if routed is not None:
        outs, info = (list(x) for x in zip(*routed))
    else:
        got = bb.eigh_batched_direct(srcs, vectors, return_info)
        outs, info = got if return_info else (got, None)
    outs = _eigh_finish(bb, outs if vectors else [(w, None) for w, _ in outs], sort)
    return (outs, info) if return_info else outs


def complex_eigh_embedded(bb, srcs, return_info=False):
    """np.linalg.eigh of complex Hermitian blocks on the float64 block engine: the one-sided block-Jacobi iteration
    of the real path on the rows of M(H) + shift (exactly structured: no QR step is involved) with the structured
    pivot solves of `CYB_EIGH_EMBEDDED_COMPLEX`.  Every eigenvalue comes out twice; real column 2a of the
    eigenvector matrix is complex eigenvector a.  Returns ([(w, V)], info), or None where the engine refuses the list."""
    Ms = embed_complex(bb, srcs)
    real = _eigh_outs(bb, Ms, True, False)
    st, info = _eigh_launch(bb, Ms, real, False, True, embedded=True)
    if st == _lib.CYB_ERR_UNSUPPORTED:
        return None
    _lib.check(st)
    outs = _eigh_outs(bb, srcs, True, True)
    bb.lincomb_many([it for (_, V), (_, v) in zip(real, outs) for it in extract_complex_items(bb, V, v)])
    bb.copy_many([(w, _view(bb, W, 0, w.shape, (2,))) for (W, _), (w, _) in zip(real, outs)])
    return outs, info


def argsort_perm(w: np.ndarray, sort):
    """block_backend.cpp:759-781."""
    if sort not in ('m<', 'SM', 'm>', 'LM', '<', 'SR', 'SA', '>', 'LR', 'LA'):
        raise ValueError(f"Unknown sort option: '{sort}'")
    key = np.abs(w) if sort in ('m<', 'SM', 'm>', 'LM') else w
    return np.argsort(-key if sort in ('m>', 'LM', '>', 'LR', 'LA') else key, kind='stable')


def _eigh_finish(bb, outs, sort):
    """[(w, V)] in the order `sort` asks for (V may be None)."""
    if sort is None:
        return outs
    res = []
    for W, V in outs:
        perm = argsort_perm(bb.to_numpy(W), sort)
        res.append((bb._gather_axis(W, perm, 0), bb._gather_axis(V, perm, 1) if V is not None else None))
    return res
