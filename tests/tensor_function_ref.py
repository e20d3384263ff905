"""numpy side of the tests of functions of a square tensor (exp, eye, hermitian_function of cyten_amd.abelian): the dense
criterion, the numpy restatement of the device's exponential algorithm, and the numpy stand-in backend with
``matrix_exp_many`` (scipy per block, so that only the block-diagonal structure of the tensor level is under test)."""
import math

import numpy as np
import scipy.linalg

from numpy_tensor_backend import NumpyTensorBackend


class NumpyExpmBackend(NumpyTensorBackend):
    def eye_matrix(self, dim, dtype=None, device=None):
        return np.eye(dim, dtype=np.dtype(dtype) if dtype is not None else float)

    def zeros(self, shape, dtype=None, device=None):
        return np.zeros(shape, dtype=np.dtype(dtype) if dtype is not None else float)

    def matrix_exp_many(self, blocks, alpha=1.0):
        cplx = isinstance(alpha, (complex, np.complexfloating)) or any(not isinstance(b, tuple) and np.iscomplexobj(b) for b in blocks)
        outs = []
        for b in blocks:
            a = np.zeros((b[0], b[0])) if isinstance(b, tuple) else np.asarray(b)
            e = scipy.linalg.expm(alpha * a) if a.size else np.zeros(a.shape)
            outs.append(np.asarray(e, dtype=complex if cplx else float))
        return outs


class NumpyLoopBackend(NumpyTensorBackend):
    """a backend WITHOUT ``matrix_exp_many``: ``exp`` must fall back to a loop over ``matrix_exp``"""

    def zeros(self, shape, dtype=None, device=None):
        return np.zeros(shape)

    def matrix_exp(self, a):
        return scipy.linalg.expm(a)


# ------------------------------------------------------------------------------------------- dense criterion

def as_matrix(dense, k):
    """the dense array of a 2k-leg tensor as the d x d matrix from legs ``n-1 .. k`` to legs ``0 .. k-1``"""
    n = dense.ndim
    perm = list(range(k)) + list(range(n - 1, k - 1, -1))
    a = np.transpose(dense, perm)
    d = math.prod(a.shape[:k])
    return a.reshape(d, d), a.shape, perm


def from_matrix(mat, shape, perm):
    return np.transpose(mat.reshape(shape), np.argsort(perm))


def dense_function(dense, fn):
    """``fn`` of the matrix of a dense square tensor, as a dense tensor again"""
    mat, shape, perm = as_matrix(dense, dense.ndim // 2)
    return from_matrix(fn(mat), shape, perm)


def dense_exp(dense, factor=1.0):
    return dense_function(dense, lambda m: scipy.linalg.expm(factor * m))


def dense_hermitian_function(dense, f):
    def fn(m):
        w, v = np.linalg.eigh(m)
        return (v * f(w)) @ v.conj().T
    return dense_function(dense, fn)


# ------------------------------------------------------------------------------------------- the algorithm

def squarings(norm1):
    return 0 if norm1 <= 0.5 else int(math.ceil(math.log2(norm1 / 0.5)))


def expm_taylor18(a):
    """scaling + degree-18 Taylor polynomial in Horner form + squaring: what ``matrix_exp`` and the in-LDS kernel compute"""
    a = np.asarray(a)
    n = a.shape[0]
    if n == 0:
        return a.copy()
    s = squarings(np.abs(a).sum(axis=0).max())
    m = a * 0.5 ** s
    eye = np.eye(n, dtype=a.dtype)
    p = eye
    for k in range(18, 0, -1):
        p = eye + (m @ p) / k
    for _ in range(s):
        p = p @ p
    return p


def families(rng, n):
    """[(name, matrix)]: the matrix families of the device tolerance, each with ||A||_1 <= 64"""
    g = rng.standard_normal((n, n)) / np.sqrt(n)
    z = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(2 * n)
    x = rng.standard_normal((n, n))
    out = [(f'gauss*{c}', c * g) for c in (1, 3, 6)]
    out += [('symmetric', g + g.T), ('hermitian', z + z.conj().T), ('i*hermitian', 1j * (z + z.conj().T)),
            ('gate -0.05i*hermitian', -0.05j * (z + z.conj().T)), ('negative semidefinite', -5.0 * (x @ x.T) / n),
            ('strictly upper*3', 3.0 * np.triu(g, 1))]
    return [(name, a) for name, a in out if np.abs(a).sum(axis=0).max() <= 64.0]
