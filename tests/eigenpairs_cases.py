"""Criteria of the thick-restart Lanczos tests shared by tests/test_eigenpairs.py (numpy stand-in) and
tests/test_gpu_eigenpairs.py (HipBlockBackend): the same inputs (tests/direct_sum_cases.py), the same bounds.

The yardstick is the dense matrix ``case.M`` in the coordinates ``case.y(.)`` in which the inner product is the plain one."""
import numpy as np

from cyten_amd import krylov

TOL = 1e-10
MAX_RESTARTS = 200     # three times the worst case of the numpy prototype on these inputs (63): a condition, not a tolerance
# (which, num_ev, N_max)
SETTINGS = [('SA', 4, 12), ('LA', 3, 12), ('SA', 4, 24), ('LM', 3, 10), ('SA', 1, 6)]


_CASES = {}


def shared_case(bb, combo, seed, cplx):
    """direct_sum_cases.SumCase(bb, combo, seed, cplx, cplx), built once per backend and shared by the tests that only read it
    (its dense spectrum, the reference of every run on it, is computed once)"""
    import direct_sum_cases as dc
    key = (id(bb), combo, seed, cplx)
    if key not in _CASES:
        _CASES[key] = (bb, dc.SumCase(bb, combo, seed, cplx, cplx))       # (the backend is kept alive: its id stays its own)
    return _CASES[key][1]


class PartCase:
    """one part of a direct_sum_cases.SumCase as a case of its own: plain tensors (a TreeTensor, an AbelianTensor) as vectors"""

    def __init__(self, part):
        self.bb, self.H, self.psi0, self.M, self.y = part.bb, part.H, part.psi0, part.M, part.y

    def spectrum(self, k=2):
        if not hasattr(self, '_spec'):
            self._spec = np.linalg.eigh(self.M)
        return self._spec[0], self._spec[1][:, :k]


def reference_values(M, which, num_ev):
    """the first `num_ev` eigenvalues in `which` order; `M`: a Hermitian matrix, or a case -- its ``spectrum()`` is the
    eigenvalues of its block-diagonal matrix, computed block by block once per case"""
    E = M.spectrum()[0] if hasattr(M, 'spectrum') else np.linalg.eigvalsh(M)
    return E[krylov.argsort_which(E, which)[:num_ev]]


def check_pairs(case, solver, Es, vecs, which, num_ev, M=None, tol=TOL):
    """the criteria of one finished run against the dense matrix `M` (default: the case's); returns the vectors' coordinates"""
    want = reference_values(case if M is None else M, which, num_ev)
    M = case.M if M is None else M
    Es = np.asarray(Es)
    assert isinstance(Es, np.ndarray) and Es.shape == (num_ev,) and Es.dtype == np.float64 and len(vecs) == num_ev
    # the criterion of direct_sum_cases.check_ground_state, for every pair
    assert np.all(np.abs(Es - want) <= 1e-9 * np.abs(want)), (Es, want)
    Y = np.array([case.y(v) for v in vecs]).T
    # A pair is accepted with the ESTIMATE |beta s| <= tol |theta|; the true residual is allowed ten times the largest of them
    res = np.linalg.norm(M @ Y - Y * Es, axis=0)
    assert res.max() <= 10 * tol * np.abs(Es).max(), res
    assert np.abs(Y.conj().T @ Y - np.eye(num_ev)).max() <= 1e-12
    T = solver.T
    assert solver.coupling_error <= 1e-10 * np.abs(T).max()
    assert solver.restarts <= MAX_RESTARTS and solver.matvecs >= num_ev
    assert len(solver.residuals) == num_ev
    return Y


def run_and_check(case, which, num_ev, N_max, flat=None, H=None, psi0=None, M=None, **more):
    """(solver, Es, vectors, N, Y) of one run that meets the criteria"""
    opts = dict(num_ev=num_ev, which=which, N_max=N_max, tol=TOL, max_restarts=MAX_RESTARTS, **more)
    if flat is not None:
        opts['flat'] = flat
    solver = krylov.LanczosEigenpairs(case.bb, case.H if H is None else H, case.psi0 if psi0 is None else psi0, opts)
    Es, vecs, N = solver.run()
    assert N == solver.matvecs
    Y = check_pairs(case, solver, Es, vecs, which, num_ev, M)
    if which == 'SA' and M is None:
        # the lowest state is separated by more than 1 in these cases
        U = case.spectrum()[1]
        assert abs(np.vdot(U[:, 0], Y[:, 0])) >= 1.0 - 1e-7
    return solver, Es, vecs, N, Y
