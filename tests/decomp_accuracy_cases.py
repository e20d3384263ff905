"""Inputs, references and measures that hold the decompositions to the rounding level (numpy and mpmath only, no GPU).

Shared by tests/test_decomp_accuracy_model.py (LAPACK on every case, mutants), tests/test_gpu_decomp_accuracy.py and
tests/decomp_accuracy_worker.py (the HIP kernels on the same cases).

Measures.  All of them are formed in `np.longdouble` / `np.clongdouble` (eps 1.08e-19) and returned in units of
EPS = 2^-52, so that their own error is three decades below one unit:
  orth(X)   max |X^H X - 1|
  resid     max |U S Vh - A| / sigma_1;  max |Q R - A| / ||A||_2;  max |A V - V W| / ||A||_F
  values    max |S - sigma_ref| / sigma_1;  max |W - lambda_ref| / ||A||_F   (absolute: eigh shifts by 2 ||A||_F)
and the structural facts are asserted exactly.  The one cap on every measure is CAP = 1e-13 (450 EPS): the figure
DESIGN.md itself quotes for the unitarity of Q and for the Jacobi measure.  LAPACK stays below 24 EPS on every shape used
here, so the cap leaves 19x over what a correct float64 algorithm needs; the model test holds LAPACK to CAP / 8.

References whose error is negligible.
  * exact family: A = H_m[:, :k] diag(d) H_n[:, :k]^T with Sylvester Hadamard matrices H and d_i in {0} + {2^0 .. 2^-30}:
    every entry is an exact double (asserted), the singular values are exactly sqrt(m n) d_i, the singular vectors are the
    Hadamard columns, rank and null space are exact.  Other shapes: zero rows / columns around A and a permutation of rows
    and columns.  Complex: rows and columns times powers of i.  Hermitian: H diag(+-d) H^T, eigenvalues n (+-d_i).
  * mpmath at 50 digits for dense blocks with min(m, n) <= 48, once per process.
  * larger dense inputs have no reference values: orth and resid only, which are self-contained."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

EPS = 2.0 ** -52
CAP = 1e-13
CAP_EPS = CAP / EPS                     # 450.4
LD = np.longdouble
CLD = np.clongdouble
D_MIN_EXP = 30                          # d_i in {0} + {2^0 .. 2^-30}
MAX_EXTENT = 2048                       # m, n <= 2048: sums of +-d_i over up to 2^11 terms still fit 53 bits
MP_DIGITS = 50
MP_MAX = 48                             # mpmath references: min(m, n) <= 48


# ---- long-double arithmetic
def _ld(x):
    x = np.asarray(x)
    return x.astype(CLD if np.iscomplexobj(x) else LD)


def _split(x, bits=20):
    """x = hi + lo, hi a multiple of 2^-bits times a power of two >= max |x|: products of two such `hi` summed over up to
    2^12 terms are exact in float64, whatever the order of the sum."""
    scale = 2.0 ** np.ceil(np.log2(max(np.abs(x).max(), 1e-300)))
    hi = np.round(x / scale * 2.0 ** bits) * (scale / 2.0 ** bits)
    return hi, x - hi


def _matmul_ld_split(x, y):
    """x @ y for float64 matrices with an inner extent up to 4096, error below 1e-21 |x| |y|: the leading parts multiply exactly in
    float64, the three cross terms are 2^-21 smaller, and the sum is taken in long double."""
    assert x.dtype == np.float64 and y.dtype == np.float64 and x.shape[1] <= 4096
    xh, xl = _split(x)
    yh, yl = _split(y)
    return _ld(xh @ yh) + _ld(xh @ yl + xl @ yh + xl @ yl)


def matmul_ld(x, y):
    """x @ y in long double.  Real float64 products of more than 2e6 multiply-adds (up to the full Q of a 2048-row block) go
    through the exact split above instead of numpy's long-double loop: the same result to 1e-21, in a hundredth of the time."""
    if x.dtype == np.float64 and y.dtype == np.float64 and x.shape[0] * x.shape[1] * y.shape[1] > 2e6 and x.shape[1] <= 4096:
        return _matmul_ld_split(x, y)
    return _ld(x) @ _ld(y)


def orth(x):
    """max |X^H X - 1| in units of EPS."""
    k = x.shape[1]
    if k == 0:
        return 0.0
    g = matmul_ld(np.ascontiguousarray(x.conj().T), x)
    return float(np.abs(g - np.eye(k, dtype=LD)).max() / EPS)


def norm2_ld(a):
    """||A||_2, good to float64 rounding (a scale, not a measured quantity)."""
    return LD(np.linalg.norm(a, 2)) if a.size else LD(0)


# ---- cases
@dataclass
class Case:
    name: str
    a: np.ndarray                       # float64 or complex128 input
    ref: np.ndarray | None = None       # long double: singular values descending / eigenvalues ascending; None: no reference
    rank: int | None = None             # exact rank (exact family only)
    u: np.ndarray | None = None         # exact family: orthonormal range vectors (float64-exact entries times 1/sqrt(m))
    v: np.ndarray | None = None
    origin: str = 'dense'               # 'exact' | 'mpmath' | 'dense'

    @property
    def shape(self):
        return self.a.shape


def hadamard(n):
    assert n >= 1 and n & (n - 1) == 0, 'Sylvester Hadamard matrices exist for powers of two'
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def _check_d(d, k_max):
    d = np.asarray(d, dtype=np.float64)
    if d.ndim != 1 or len(d) > k_max:
        raise ValueError(f'd must be a vector of at most {k_max} entries')
    mag = np.abs(d[d != 0])
    if mag.size:
        e = np.log2(mag)
        if np.any(e != np.round(e)) or e.max() > 0 or e.min() < -D_MIN_EXP:
            raise ValueError(f'every d_i must be 0 or +-2^-j with 0 <= j <= {D_MIN_EXP}')
    return d


def _phases(n, seed):
    return (1j ** np.random.default_rng(seed).integers(0, 4, n)) if n else np.ones(0, complex)


def _exact_product(hm, d, hn):
    """hm diag(d) hn^T in float64, asserted equal to the same product formed in long double."""
    a = (hm * d) @ hn.T
    if not np.array_equal(_ld(a), (_ld(hm) * _ld(d)) @ _ld(hn).T):
        raise ValueError('the product is not exact in float64')
    return a


def _place(a, shape, seed, symmetric=False):
    """`a` in the corner of a zero matrix of `shape`, rows and columns permuted (one permutation for both if `symmetric`)."""
    m, n = a.shape
    big = np.zeros(shape, dtype=a.dtype)
    big[:m, :n] = a
    rng = np.random.default_rng(seed)
    pr = rng.permutation(shape[0])
    pc = pr if symmetric else rng.permutation(shape[1])
    return big[np.ix_(pr, pc)], pr, pc


def exact_svd_case(name, m, n, d, shape=None, cplx=False, seed=0):
    """A = H_m[:, :k] diag(d) H_n[:, :k]^T, m and n powers of two <= 2048, optionally inside zero rows / columns up to `shape`
    and permuted, optionally with rows and columns times powers of i.  Raises ValueError on a d outside the exact range."""
    if max(m, n) > MAX_EXTENT:
        raise ValueError(f'm, n must not exceed {MAX_EXTENT}')
    d = _check_d(d, min(m, n))
    if np.any(d < 0):
        raise ValueError('singular values are not negative')
    k = len(d)
    hm, hn = hadamard(m)[:, :k], hadamard(n)[:, :k]
    a = _exact_product(hm, d, hn)
    u, v = hm / np.sqrt(LD(m)), hn / np.sqrt(LD(n))
    shape = shape or (m, n)
    if shape != (m, n):
        a, pr, pc = _place(a, shape, seed)
        ub, vb = np.zeros((shape[0], k), dtype=LD), np.zeros((shape[1], k), dtype=LD)
        ub[:m], vb[:n] = u, v
        u, v = ub[pr], vb[pc]
    if cplx:
        fr, fc = _phases(shape[0], seed + 1), _phases(shape[1], seed + 2)
        a = fr[:, None] * a * fc[None, :]
        u, v = _ld(fr)[:, None] * u, np.conj(_ld(fc))[:, None] * v     # A = U S V^H
    ref = np.zeros(min(shape), dtype=LD)
    ref[:k] = np.sqrt(LD(m) * LD(n)) * _ld(d)
    ref = np.sort(ref)[::-1]
    order = np.argsort(-d, kind='stable')
    rank = int(np.count_nonzero(d))
    return Case(name, a, ref, rank, u[:, order][:, :rank], v[:, order][:, :rank], 'exact')


def exact_eigh_case(name, n, d, shape=None, cplx=False, seed=0):
    """A = H_n[:, :k] diag(d) H_n[:, :k]^T with signed d: eigenvalues n d_i and n - k zeros; `shape` and `cplx` as above (one
    permutation and one set of phases for rows and columns: the result stays Hermitian)."""
    if n > MAX_EXTENT:
        raise ValueError(f'n must not exceed {MAX_EXTENT}')
    d = _check_d(d, n)
    h = hadamard(n)[:, :len(d)]
    a = _exact_product(h, d, h)
    size = shape or n
    if size != n:
        a, _, _ = _place(a, (size, size), seed, symmetric=True)
    if cplx:
        f = _phases(size, seed + 1)
        a = f[:, None] * a * np.conj(f)[None, :]
    ref = np.zeros(size, dtype=LD)
    ref[:len(d)] = LD(n) * _ld(d)
    return Case(name, a, np.sort(ref), int(np.count_nonzero(d)), origin='exact')


# ---- spectra of the exact family (k entries, `r` of them non-zero)
def d_full(k, r=None):
    """Condition 8, every value k/4-fold."""
    r = k if r is None else r
    return np.r_[2.0 ** -(np.arange(r) % 4), np.zeros(k - r)]


def d_eightfold(k, r=None):
    r = k if r is None else r
    return np.r_[2.0 ** -((np.arange(r) // 8) % (D_MIN_EXP + 1)), np.zeros(k - r)]


def d_cluster(k, r=None):
    """One cluster of k/4 ones next to graded values 2^-1 .. 2^-30."""
    r = k if r is None else r
    c = min(k // 4, r)
    return np.r_[np.ones(c), 2.0 ** -(1 + np.arange(r - c) % D_MIN_EXP), np.zeros(k - r)]


def d_graded(k, r=None):
    """2^0 .. 2^-30, evenly spread over the non-zero entries."""
    r = k if r is None else r
    return np.r_[2.0 ** -np.floor(np.arange(r) * (D_MIN_EXP + 1) / r), np.zeros(k - r)]


def d_signed(n):
    """Hermitian family: +- pairs of equal magnitude, one eightfold eigenvalue, n/2 exact zeros."""
    r = n // 2
    mag = np.r_[np.full(8, 0.5), 2.0 ** -(np.arange(r - 8) // 2 % 8)]
    sign = np.r_[np.ones(8), np.where(np.arange(r - 8) % 2 == 0, 1.0, -1.0)]
    return np.r_[mag * sign, np.zeros(n - r)]


# ---- mpmath references
def _mp():
    import mpmath
    mpmath.mp.dps = MP_DIGITS
    return mpmath


def _to_ld(values):
    mp = _mp()
    return np.array([LD(mp.nstr(x, 30)) for x in values], dtype=LD)


def _mp_matrix(a):
    mp = _mp()
    if np.iscomplexobj(a):
        return mp.matrix([[mp.mpc(float(z.real), float(z.imag)) for z in row] for row in a])
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in a])


def mp_singular_values(a):
    """Singular values of `a`, descending, as mpmath numbers at 50 digits."""
    mp = _mp()
    s = (mp.svd_c if np.iscomplexobj(a) else mp.svd_r)(_mp_matrix(a), compute_uv=False)
    return sorted((s[i] for i in range(len(s))), reverse=True)


def mp_eigenvalues(a):
    mp = _mp()
    w = (mp.eighe if np.iscomplexobj(a) else mp.eigsy)(_mp_matrix(a), eigvals_only=True)
    return sorted(w[i] for i in range(len(w)))


def crandn(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _dense(shape, seed, cplx=False):
    rng = np.random.default_rng(seed)
    return crandn(rng, shape) if cplx else rng.standard_normal(shape)


def _herm(n, seed, cplx=False):
    z = _dense((n, n), seed, cplx)
    return z + z.conj().T


@functools.lru_cache(maxsize=None)
def mp_svd_case(m, n, cplx=False, seed=0):
    a = _dense((m, n), 1000 + 7 * m + n + seed, cplx)
    assert min(m, n) <= MP_MAX
    return Case(f'mpmath {"c" if cplx else "r"} {m}x{n}', a, _to_ld(mp_singular_values(a)), origin='mpmath')


@functools.lru_cache(maxsize=None)
def mp_eigh_case(n, cplx=False, seed=0):
    a = _herm(n, 2000 + n + seed, cplx)
    assert n <= MP_MAX
    return Case(f'mpmath {"c" if cplx else "r"} {n}x{n}', a, _to_ld(mp_eigenvalues(a)), origin='mpmath')


def gaussian(m, n, seed, cplx=False):
    return Case(f'gaussian {m}x{n}', _dense((m, n), seed, cplx))


def low_rank_noise(m, n, r, noise, seed, cplx=False):
    rng = np.random.default_rng(seed)
    f = (lambda s: crandn(rng, s)) if cplx else rng.standard_normal
    return Case(f'rank {r} + {noise:g} noise {m}x{n}', f((m, r)) @ f((r, n)) + noise * f((m, n)))


def theta_like(m, n, r, seed, cplx=False):
    rng = np.random.default_rng(seed)
    f = (lambda s: crandn(rng, s)) if cplx else rng.standard_normal
    return Case(f'theta {m}x{n} rank {r}', f((m, r)) @ f((r, n)))


# ---- measures and the checks that hold a result to the cap
class AccuracyError(AssertionError):
    pass


def _fail(case, what):
    raise AccuracyError(f'{case.name} {case.shape}: {what}')


def _hold(case, measures, cap_eps, caps=None):
    """Every measure <= cap_eps; `caps`: {measure: its own cap in EPS}, for the cases DESIGN.md lists with their cause."""
    for key, val in measures.items():
        cap = (caps or {}).get(key, cap_eps)
        if not val <= cap:               # (NaN fails)
            _fail(case, f'{key} = {val:.1f} eps exceeds {cap:.1f} eps; all: ' + format_measures(measures))
    return measures


def format_measures(measures):
    return '  '.join(f'{k} {v:9.2f}' for k, v in measures.items())


def table_line(route, case, measures):
    """One line per case: route, shape, orth_u, orth_v, resid, values (in EPS; '-' where a measure does not apply)."""
    cols = ' '.join(f'{measures[k]:9.2f}' if k in measures else f'{"-":>9s}' for k in ('orth_u', 'orth_v', 'resid', 'values'))
    shape = 'x'.join(str(s) for s in case.shape)
    return f'[accuracy] {route:28s} {case.name:34s} {shape:>10s} {cols}'


def svd_measures(case, U, S, Vh):
    a = case.a
    m, n = a.shape
    k = min(m, n)
    cplx = np.iscomplexobj(a)
    if U.shape != (m, k) or S.shape != (k,) or Vh.shape != (k, n):
        _fail(case, f'shapes {U.shape} {S.shape} {Vh.shape}')
    want = np.complex128 if cplx else np.float64
    if U.dtype != want or Vh.dtype != want or S.dtype != np.float64:
        _fail(case, f'dtypes {U.dtype} {S.dtype} {Vh.dtype}')
    if not np.all(S >= 0):
        _fail(case, 'S has a negative (or NaN) entry')
    if not np.all(S[:-1] >= S[1:]):
        _fail(case, 'S is not descending')
    out = {'orth_u': orth(U), 'orth_v': orth(np.ascontiguousarray(Vh.conj().T))}
    if k == 0:
        return out
    s1 = LD(case.ref[0]) if case.ref is not None else LD(S[0])
    if s1 == 0:                          # the zero matrix: absolute measures
        s1 = LD(1)
    out['resid'] = float(np.abs((_ld(U) * _ld(S)) @ _ld(Vh) - _ld(a)).max() / s1 / EPS)
    if case.ref is not None:
        out['values'] = float(np.abs(_ld(S) - case.ref).max() / s1 / EPS)
    return out


def check_svd(case, U, S, Vh, cap_eps=CAP_EPS, caps=None):
    return _hold(case, svd_measures(case, U, S, Vh), cap_eps, caps)


INDIVIDUAL_CAP_MAX = 1e-11 / EPS        # no individual cap is looser than this; at most two cases carry one


def complex_jacobi_null_cap(case):
    """The rank threshold of the complex Jacobi kernels (csvd_large.hip: a column of norm <= 2.3e-16 M ||A||_F is a null
    direction and keeps its computed norm as its singular value), relative to sigma_1, in EPS."""
    fro = np.sqrt((np.abs(_ld(case.a)) ** 2).sum())
    cap = float(2.3e-16 * max(case.shape) * fro / case.ref[0] / EPS)
    assert CAP_EPS < cap <= INDIVIDUAL_CAP_MAX
    return cap


def eigh_measures(case, W, V):
    a = case.a
    n = a.shape[0]
    cplx = np.iscomplexobj(a)
    if W.shape != (n,) or V.shape != (n, n):
        _fail(case, f'shapes {W.shape} {V.shape}')
    if W.dtype != np.float64 or V.dtype != (np.complex128 if cplx else np.float64):
        _fail(case, f'dtypes {W.dtype} {V.dtype}')
    if not np.all(W[:-1] <= W[1:]):
        _fail(case, 'W is not ascending')
    out = {'orth_v': orth(V)}
    if n == 0:
        return out
    fro = np.sqrt((np.abs(_ld(a)) ** 2).sum())
    if fro == 0:
        fro = LD(1)
    out['resid'] = float(np.abs(_ld(a) @ _ld(V) - _ld(V) * _ld(W)).max() / fro / EPS)
    if case.ref is not None:
        out['values'] = float(np.abs(_ld(W) - case.ref).max() / fro / EPS)
    return out


def check_eigh(case, W, V, cap_eps=CAP_EPS):
    return _hold(case, eigh_measures(case, W, V), cap_eps)


def qr_measures(case, Q, R, full=False, positive_diagonal=False):
    a = case.a
    m, n = a.shape
    kq = m if full else min(m, n)
    if Q.shape != (m, kq) or R.shape != (kq, n):
        _fail(case, f'shapes {Q.shape} {R.shape}')
    if Q.dtype != a.dtype or R.dtype != a.dtype:
        _fail(case, f'dtypes {Q.dtype} {R.dtype}')
    if np.any(np.tril(R, -1) != 0):
        _fail(case, 'R has a non-zero entry below its diagonal')
    if positive_diagonal:
        dg = np.diagonal(R)
        if not (np.all(dg.real >= 0) and np.all(dg.imag == 0)):
            _fail(case, 'diag(R) is not real and non-negative')
    out = {'orth_u': orth(Q)}
    if m * n == 0:
        return out
    nrm = norm2_ld(a)
    if nrm == 0:
        nrm = LD(1)
    out['resid'] = float(np.abs(matmul_ld(np.ascontiguousarray(Q), np.ascontiguousarray(R)) - _ld(a)).max() / nrm / EPS)
    return out


def check_qr(case, Q, R, full=False, positive_diagonal=False, cap_eps=CAP_EPS):
    return _hold(case, qr_measures(case, Q, R, full, positive_diagonal), cap_eps)


# ---- the case lists, by the route each list is built to reach (tests/test_gpu_decomp_accuracy.py states how)
def svd_real_groups():
    g = {}
    # every block fits the in-LDS kernel (min <= 64, max <= 128): the list as a whole runs svd_small.hip
    g['in-LDS'] = (
        [gaussian(m, n, 11 + i) for i, (m, n) in enumerate([(1, 1), (2, 1), (7, 5), (33, 127), (64, 64), (128, 64), (63, 64)])]
        + [exact_svd_case(f'exact {tag} {m}x64', m, 64, d) for m in (64, 128)
           for tag, d in (('full', d_full(64)), ('rank 32', d_full(64, 32)), ('cluster', d_cluster(64)), ('eightfold', d_eightfold(64)))]
        + [exact_svd_case('exact graded 63x64', 32, 32, d_graded(32), shape=(63, 64), seed=3)]
        + [mp_svd_case(7, 5), mp_svd_case(33, 33), mp_svd_case(48, 48), mp_svd_case(30, 90)])
    # fewer than 16 fitting blocks beside one that does not fit: every block with min >= 2 joins the pipeline
    g['tiny blocks in the pipeline'] = [mp_svd_case(7, 5), mp_svd_case(33, 33), gaussian(70, 70, 21)]
    g['pipeline, no deflation'] = [gaussian(70, 70, 22), gaussian(130, 66, 23), low_rank_noise(130, 66, 20, 1e-8, 24),
                                   exact_svd_case('exact full 70x70', 64, 64, d_full(64), shape=(70, 70), seed=5)]
    g['pipeline, deflation and completion'] = [
        exact_svd_case('exact rank 64 128x128', 128, 128, d_full(128, 64)),
        exact_svd_case('exact rank 96 256x128', 256, 128, d_eightfold(128, 96)),
        theta_like(150, 130, 60, 25), low_rank_noise(140, 200, 30, 1e-12, 26)]
    g['pipeline, early stop off a panel boundary'] = [exact_svd_case('exact rank 150 256x256', 256, 256, d_full(256, 150))]
    g['pipeline, panels of more than 1536 rows'] = [exact_svd_case('exact k 48 2048x64', 2048, 64, d_cluster(64, 48)),
                                                    exact_svd_case('exact k 48 64x2048', 64, 2048, d_cluster(64, 48))]
    return g


def svd_r0_cases():
    """Exact 256 x 256 blocks with 144 or 176 non-zero values (r0 rows left after the first QR).  Whether a block accumulates
    its rotations or recovers them is decided per process (CYB_SVD_JREC_MIN: 256 by default, 160 in one variant of the worker,
    between the two ranks), and by the spread of its row norms: the graded blocks are refused the recovery up front."""
    out = []
    for r0 in (144, 176):
        out += [exact_svd_case(f'exact full r0 {r0}', 256, 256, d_full(256, r0)),
                exact_svd_case(f'exact graded r0 {r0}', 256, 256, d_graded(256, r0))]
    return out


def svd_complex_groups():
    g = {}
    g['csvd_small'] = ([mp_svd_case(12, 7, True), mp_svd_case(40, 40, True)]
                       + [exact_svd_case(f'exact {tag} 64x64', 64, 64, d, cplx=True, seed=31)
                          for tag, d in (('full', d_full(64)), ('rank 32', d_full(64, 32)), ('eightfold', d_eightfold(64)))])
    g['csvd_large'] = [exact_svd_case('exact full 80x80', 64, 64, d_full(64), shape=(80, 80), cplx=True, seed=32),
                       exact_svd_case('exact rank 40 80x80', 64, 64, d_full(64, 40), shape=(80, 80), cplx=True, seed=33),
                       exact_svd_case('exact full 90x70', 64, 64, d_full(64), shape=(90, 70), cplx=True, seed=34),
                       exact_svd_case('exact rank 40 90x70', 64, 64, d_full(64, 40), shape=(90, 70), cplx=True, seed=35),
                       gaussian(80, 80, 36, True), gaussian(90, 70, 37, True)]
    g['embedded'] = [exact_svd_case('exact full 128x128', 128, 128, d_full(128), cplx=True, seed=38),
                     exact_svd_case('exact eightfold 128x128', 128, 128, d_eightfold(128), cplx=True, seed=39),
                     exact_svd_case('exact rank 64 256x128', 256, 128, d_full(128, 64), cplx=True, seed=40),
                     gaussian(128, 100, 41, True)]
    return g


def eigh_groups():
    g = {}
    g['real in-LDS'] = [mp_eigh_case(9), mp_eigh_case(48), exact_eigh_case('exact signed 64', 64, d_signed(64)),
                        Case('hermitian 33', _herm(33, 51)), Case('hermitian 1', _herm(1, 52))]
    g['real engine'] = [exact_eigh_case(f'exact signed {n}', n, d_signed(n)) for n in (128, 256)] + [Case('hermitian 100', _herm(100, 53))]
    g['complex small'] = [mp_eigh_case(9, True), mp_eigh_case(40, True),
                          exact_eigh_case('exact signed 64', 64, d_signed(64), cplx=True, seed=54)]
    g['complex large'] = [exact_eigh_case('exact signed 80', 64, d_signed(64), shape=80, cplx=True, seed=55),
                          Case('hermitian 90', _herm(90, 56, True))]
    g['complex embedded'] = [exact_eigh_case(f'exact signed {n}', n, d_signed(n), cplx=True, seed=57 + n) for n in (128, 256)]
    return g


def qr_real_cases():
    return [gaussian(20, 20, 61), gaussian(130, 250, 62), gaussian(300, 120, 63), gaussian(2048, 64, 64),
            low_rank_noise(300, 120, 40, 1e-5, 65),
            exact_svd_case('exact rank 64 256x128', 256, 128, d_full(128, 64))]


def qr_complex_groups():
    g = {}
    g['one-workgroup kernel'] = [gaussian(40, 40, 71, True), gaussian(96, 30, 72, True), gaussian(30, 96, 73, True)]
    # more than 96 x 96 elements in the working copy: one launch per column step.  The router keeps such blocks for the embedded
    # route unless min < 48 and max <= 128 (then only a full Q is large enough), so the test hands these to the direct entry
    g['step kernel'] = [gaussian(120, 40, 74, True), gaussian(130, 100, 75, True), gaussian(100, 131, 79, True)]
    g['embedded'] = [gaussian(130, 100, 75, True), gaussian(257, 255, 76, True), gaussian(48, 48, 77, True)]
    g['embedded, rank deficient'] = [exact_svd_case('exact rank 64 128x128', 128, 128, d_full(128, 64), cplx=True, seed=78)]
    return g


def worker_cases():
    """The compact list of tests/decomp_accuracy_worker.py: {kind: [cases]}."""
    real = svd_real_groups()
    return {
        'svd': [gaussian(70, 70, 22), gaussian(130, 66, 23)] + real['pipeline, deflation and completion'][:2]
               + real['pipeline, early stop off a panel boundary'] + real['pipeline, panels of more than 1536 rows'] + svd_r0_cases(),
        'csvd': svd_complex_groups()['embedded'][:3],
        'eigh': eigh_groups()['real engine'][:2],
        'ceigh': eigh_groups()['complex embedded'][:1],
    }


def all_cases():
    """Every case of the module once, as (kind, case); kind in 'svd', 'eigh', 'qr'."""
    seen, out = set(), []

    def add(kind, cases):
        for c in cases:
            key = (kind, c.name, c.shape, c.a.dtype.str)
            if key not in seen:
                seen.add(key)
                out.append((kind, c))
    for grp in (svd_real_groups(), svd_complex_groups()):
        for cases in grp.values():
            add('svd', cases)
    add('svd', svd_r0_cases())
    for cases in eigh_groups().values():
        add('eigh', cases)
    add('qr', qr_real_cases())
    for cases in qr_complex_groups().values():
        add('qr', cases)
    return out
