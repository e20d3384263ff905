"""numpy model of the wide application of Q (csrc/blocked_qr.hip, `apply_q_wide` / `merge_t_kernel`): the 32-column
compact-WY factors of a blocked Householder QR are merged into one W-wide factor per group of panels,

    T_S[0:a, a:a+w_b] = -T_S[0:a, 0:a] (V_S[:, 0:a]^T V_S[:, a:a+w_b]) T_b     (diagonal blocks: the stored T_b),

and Q is applied group by group, C[j0:, :] -= (V_S T_S) (V_S^T C[j0:, :]), last group first.  Both routes apply the same
orthogonal matrix, so they may differ by rounding only: at most 1e-12 max|C| here (measured 4e-15 ... 1.1e-14)."""
import numpy as np
import pytest
import scipy.linalg

NBK = 32


def _factor(a, n_fac=None):
    """Explicit reflectors V (unit lower trapezoidal, zeros above each panel) and the 32 x 32 factors T of every panel
    (dlarft, forward columnwise) from LAPACK's dgeqrf; panels at or behind `n_fac` are the identity (T = 0)."""
    m, n = a.shape
    k = min(m, n)
    (qr, tau), _ = scipy.linalg.qr(a, mode='raw')
    V = np.tril(qr[:, :k], -1)
    V[np.arange(k), np.arange(k)] = 1.0
    Ts = []
    for p, j0 in enumerate(range(0, k, NBK)):
        pw = min(NBK, k - j0)
        T = np.zeros((NBK, NBK))
        for j in range(pw):
            T[j, j] = tau[j0 + j]
            T[:j, j] = -tau[j0 + j] * T[:j, :j] @ (V[:, j0:j0 + j].T @ V[:, j0 + j])
        if n_fac is not None and p >= n_fac:
            T[:] = 0.0
        Ts.append(T)
    return V, Ts


def _apply_panels(V, Ts, C):
    C = C.copy()
    k = V.shape[1]
    for p in reversed(range(len(Ts))):
        j0 = p * NBK
        pw = min(NBK, k - j0)
        Vp = V[j0:, j0:j0 + pw]
        C[j0:] -= Vp @ (Ts[p][:pw, :pw] @ (Vp.T @ C[j0:]))
    return C


def _merge(V, Ts, j0, w):
    """T_S of the group of columns [j0, j0 + w)."""
    VS = V[j0:, j0:j0 + w]
    TS = np.zeros((w, w))
    for b, a in enumerate(range(0, w, NBK)):
        wb = min(NBK, w - a)
        Tb = Ts[j0 // NBK + b][:wb, :wb]
        TS[a:a + wb, a:a + wb] = Tb
        if a:
            TS[:a, a:a + wb] = -TS[:a, :a] @ (VS[:, :a].T @ VS[:, a:a + wb]) @ Tb
    return TS


def _apply_wide(V, Ts, C, W):
    C = C.copy()
    k = V.shape[1]
    for j0 in reversed(range(0, k, W)):
        w = min(W, k - j0)
        VS = V[j0:, j0:j0 + w]
        C[j0:] -= (VS @ _merge(V, Ts, j0, w)) @ (VS.T @ C[j0:])
    return C


@pytest.mark.parametrize('m,n,rank,W', [(200, 136, None, 128), (160, 160, 70, 128), (300, 260, 120, 64), (96, 40, None, 128),
                                        (333, 200, None, 96)])
def test_merged_factors_apply_the_same_q(m, n, rank, W):
    rng = np.random.default_rng(m * 1000 + n)
    if rank is None:
        a, n_fac = rng.standard_normal((m, n)), None
    else:
        a = rng.standard_normal((m, rank)) @ rng.standard_normal((rank, n))
        n_fac = -(-rank // NBK)     # the T of every panel at or behind ceil(rank / 32) is zero
    V, Ts = _factor(a, n_fac)
    C = 4.0 * rng.uniform(-1.0, 1.0, (m, 77))
    ref = _apply_panels(V, Ts, C)
    got = _apply_wide(V, Ts, C, W)
    diff = np.abs(got - ref).max()
    print(f'm={m} n={n} rank={rank} W={W}: max difference {diff:.2e}, max|C| {np.abs(C).max():.2f}')
    assert diff <= 1e-12 * np.abs(C).max()
    if n_fac is None:   # ... and it is Q: against LAPACK's own application
        (qr, tau), _ = scipy.linalg.qr(a, mode='raw')
        want = scipy.linalg.lapack.dormqr('L', 'N', qr[:, :min(m, n)], tau, C, max(1, 64 * 77))[0]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(C).max()
