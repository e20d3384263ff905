"""numpy restatement of the Krylov solvers on fusion-tree vectors in SCALED COORDINATES y_c = sqrt(d_c) vec(X_c) (row-major
vec, one segment per coupled sector c with quantum dimension d_c): there the weighted inner product
sum_c d_c <X_c, Y_c> is the plain one, X -> A X B is the dense matrix (+)_c kron(A_c, B_c^T), and every solver has its
textbook dense form.  Shared by tests/test_tree_krylov.py and tests/test_gpu_tree_krylov.py."""
import numpy as np
import scipy.linalg as sla


def scaled(blocks, qdims):
    """y of a vector given as one block (or None: zero) per coupled sector; `shapes` are taken from the blocks"""
    return np.concatenate([np.sqrt(d) * np.asarray(b).ravel() for b, d in zip(blocks, qdims)])


def unscaled(y, shapes, qdims):
    out, off = [], 0
    for sh, d in zip(shapes, qdims):
        n = sh[0] * sh[1]
        out.append(y[off:off + n].reshape(sh) / np.sqrt(d))
        off += n
    return out


def sector_matrices(A, B):
    """kron(A_c, B_c^T) per coupled sector: vec_row(A X B) = kron(A, B^T) vec_row(X)"""
    return [np.kron(a, b.T) for a, b in zip(A, B)]


def dense_operator(A, B):
    return sla.block_diag(*sector_matrices(A, B))


def lanczos_h(M, y0, N):
    """the (N + 1) x (N + 1) tridiagonal matrix of N Lanczos steps with full reorthogonalisation, the recurrences of
    LanczosGroundState._build_krylov (krylov_based.cpp:855-890) written out on dense vectors"""
    h = np.zeros((N + 1, N + 1))
    w = np.array(y0, dtype=np.result_type(M.dtype, y0.dtype))
    beta = np.linalg.norm(w)
    cache = []
    for k in range(N):
        w = w / beta
        cache.append(w)
        w = M @ w
        alpha = float(np.real(np.vdot(w, cache[-1])))
        h[k, k] = alpha
        w = w - alpha * cache[-1]
        for v in cache[:-1]:
            w = w - np.vdot(v, w) * v
        beta = np.linalg.norm(w)
        h[k, k + 1] = h[k + 1, k] = beta
    return h


def expm_apply(A, B, delta, y):
    """exp(delta M) y with scipy.linalg.expm, sector by sector (M is their direct sum)"""
    out, off = [], 0
    for m in sector_matrices(A, B):
        n = m.shape[0]
        out.append(sla.expm(delta * m) @ y[off:off + n])
        off += n
    return np.concatenate(out)


def weighted_qr(V, d):
    """rows of V orthonormalised in the inner product sum_i d_i conj(a_i) b_i"""
    s = np.sqrt(d)
    q = np.linalg.qr((V * s).T)[0].T
    return np.ascontiguousarray(q / s)
