"""CPU model of the rotation recovery of the batched SVD ("rotation recovery").

The LQ branch of ``run_svd_qr`` iterates on the triangle ``R2`` (``R_g^T = Q2 R2``).  With the rotations not
accumulated, the sweeps leave ``W_f = J' R2 = S Z^T`` and the factor the read-off needs is recovered afterwards,

    J' = S^-2 W_f R2^T        (= (R2 Z S^-1)^T : one triangular x dense product and a row scaling).

This file restates that in numpy, together with the rule that decides BEFORE the sweeps which blocks take the route
(``jrec_admits``: ``wants_jrec`` and the constants of ``svd_plan.h``), and pins where the default of ``CYB_SVD_JREC_RATIO`` comes
from: the largest power of ten for which every block the rule admits is recovered at least 10x inside the bound the
device checks (``JREC_BOUND``), and for which the 12- and 14-decade blocks are refused.

The converged rows are LAPACK's (``numpy.linalg.svd(R2)``), not the device iteration's; the device adds its own
isometry drift of W (2e-12), which is why the device bound sits 5x inside the project's 1e-10.
"""
import numpy as np
import pytest

EPS = 2.220446049250313e-16
# ---- the constants of svd_plan.h (kept in step by test_constants_match_the_source)
JREC_BOUND = 2e-11   # device: max |J' J'^T - 1| above this -> the list is redone with accumulation
JREC_RATIO = 1e1     # CYB_SVD_JREC_RATIO default
JREC_MIN = 256       # CYB_SVD_JREC_MIN default


def _orth(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _graded(rng, n, decades):
    return (_orth(rng, n) * np.logspace(0, -decades, n)) @ _orth(rng, n).T


def families():
    """name -> matrix; seeded, the sizes of the table in DESIGN 4.2."""
    rng = np.random.default_rng(20240611)
    out = {}
    out['theta 1024 (rank 512)'] = rng.standard_normal((1024, 512)) @ rng.standard_normal((512, 1024)) / 512 ** 0.5
    out['gaussian 1024'] = rng.standard_normal((1024, 1024))
    for d in (4, 8, 9, 10, 11, 12, 14):
        out[f'spectrum {d} decades 512'] = _graded(rng, 512, d)
    out['columns 8 decades 512'] = rng.standard_normal((512, 512)) * np.logspace(0, -8, 512)
    z = rng.standard_normal((462, 600))
    z[rng.choice(462, 140, replace=False), :] = 0.0  # (wide: the factored A^T has 140 zero columns)
    out['zero columns 462x600'] = z
    t = rng.standard_normal((1024, 512)) @ rng.standard_normal((512, 1024)) / 512 ** 0.5
    t[:, rng.choice(100, 5, replace=False)] = 0.0   # a zero column among the first: one more row of R than the rank
    out['theta 1024, zero columns'] = t
    s = np.linspace(2.0, 1.0, 256)
    s[100:110] = 1.5  # an exactly repeated singular value (ten-fold)
    out['repeated value 256'] = (_orth(rng, 256) * s) @ _orth(rng, 256).T
    return out


def precondition(A):
    """A -> QR -> up-front deflation at numpy's rank tolerance -> LQ.  Returns (R2, row norms of the surviving rows of R,
    thr2): what the device holds when it decides, and the triangle it iterates on."""
    m, n = A.shape
    if m < n:
        A = A.T
    R = np.linalg.qr(A, mode='r')
    rn = np.linalg.norm(R, axis=1)
    thr2 = (rn ** 2).sum() * (max(m, n) * EPS) ** 2
    good = rn ** 2 > thr2
    R2 = np.linalg.qr(R[good].T, mode='r')
    return R2, rn[good], thr2


def jrec_admits(row_norms, r0, ratio=JREC_RATIO, rmin=JREC_MIN):
    """The rule of run_svd_qr: spread of the surviving row norms of R (what the host already holds) and a minimum size."""
    return r0 >= rmin and row_norms.max() <= ratio * row_norms.min()


SWEEPS = 10   # what the iteration needs on these families


def row_error(r0):
    """Relative error the iteration leaves in a row of S Z^T.  LAPACK's rows are exact to a few eps; the device's are not:
    every round applies a 32 x 32 orthogonal factor, itself accurate to eps per entry, to the pair's 32 rows, and a row
    goes through (r0 / 16 - 1) rounds per sweep.  Errors of independent rounds add as a random walk:
    eps * sqrt(32 * rounds * sweeps) -- 3e-14 at r0 = 1024."""
    return EPS * np.sqrt(32.0 * max(r0 / 16 - 1, 1) * SWEEPS)


def recover(R2, rng):
    """-> (max |J' J'^T - 1|, squared row norms) with the converged rows from LAPACK, perturbed row by row by the relative
    error of the device iteration.  The recovery multiplies that error by up to the condition of R2 -- the accumulated J'
    never sees it -- and this, not the rounding of the product itself, is what limits the route."""
    _, s, zt = np.linalg.svd(R2)
    Wf = s[:, None] * zt
    g = rng.standard_normal(Wf.shape)
    Wf = Wf + row_error(len(s)) * s[:, None] * g / np.linalg.norm(g, axis=1)[:, None]
    sig2 = (Wf ** 2).sum(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        J = (Wf @ np.triu(R2).T) / sig2[:, None]
    return np.abs(J @ J.T - np.eye(len(s))).max(), sig2


@pytest.fixture(scope='module')
def table():
    rows = {}
    rng = np.random.default_rng(7)
    for name, A in families().items():
        R2, rn, thr2 = precondition(A)
        dev, sig2 = recover(R2, rng)
        rn2 = np.linalg.norm(R2, axis=1)
        rows[name] = dict(r0=len(rn), ratio_R=rn.max() / rn.min(), ratio_R2=rn2.max() / rn2.min(),
                          cond=np.sqrt(sig2.max() / max(sig2.min(), 1e-300)), dev=dev, null=bool((sig2 <= thr2).any()))
        print(f'{name:28s} r0 {len(rn):4d}  rows(R) hi/lo {rows[name]["ratio_R"]:.1e}  rows(R2) hi/lo {rows[name]["ratio_R2"]:.1e}'
              f'  cond {rows[name]["cond"]:.1e}  dev {dev:.1e}  null row {rows[name]["null"]}')
    return rows


def _holds(table, ratio):
    """Every admitted block without a null row (those are redone on the device: 'bad') is 10x inside the bound; a block
    that is not must be refused with a factor 10 to spare in the predictor, because the spread of the row norms of R
    follows the condition of R2 only within that factor (the 'cond' column against 'rows(R)': 1.4 to 30)."""
    for name, r in table.items():
        if r['r0'] < JREC_MIN or r['null']:
            continue
        inside = r['dev'] <= JREC_BOUND / 10
        if not inside and r['ratio_R'] <= 10 * ratio:
            return False
        if r['ratio_R'] <= ratio and ('12 decades' in name or '14 decades' in name):
            return False
    return True


def test_admitted_blocks_are_recovered_inside_the_bound(table):
    for name, r in table.items():
        if r['r0'] >= JREC_MIN and r['ratio_R'] <= JREC_RATIO and not r['null']:
            assert r['dev'] <= JREC_BOUND / 10, (name, r)


def test_graded_blocks_are_refused(table):
    for name in ('spectrum 12 decades 512', 'spectrum 14 decades 512'):
        assert not (table[name]['ratio_R'] <= JREC_RATIO), (name, table[name])


def test_benchmark_kind_is_admitted(table):
    r = table['theta 1024 (rank 512)']
    assert r['ratio_R'] <= JREC_RATIO and r['dev'] <= 1e-13


def test_zero_columns_are_caught_by_the_null_row_rule(table):
    # R has zero columns but no small row: the spread of its row norms does not show the deficiency, the rows of S Z^T do
    assert table['zero columns 462x600']['null']
    # ... and this one is admitted up front: the case of the 'recovered then redone' route
    r = table['theta 1024, zero columns']
    assert r['r0'] >= JREC_MIN and r['ratio_R'] <= JREC_RATIO and r['null']


def test_repeated_value_recovers(table):
    r = table['repeated value 256']
    assert r['ratio_R'] <= JREC_RATIO and not r['null'] and r['dev'] <= 1e-13


def test_default_ratio_is_the_largest_power_of_ten_that_holds(table):
    best = max(p for p in range(0, 16) if all(_holds(table, 10.0 ** q) for q in range(0, p + 1)))
    print('largest power of ten that holds: 1e%d' % best)
    assert 10.0 ** best == JREC_RATIO


def test_constants_match_the_source():
    import os
    import re
    # (the bound and the defaults of SvdSwitches: the member initialisers)
    src = open(os.path.join(os.path.dirname(__file__), '..', 'cyten_amd', 'csrc', 'svd_plan.h')).read()
    assert float(re.search(r'JREC_BOUND\s*=\s*([0-9.e+-]+)', src).group(1)) == JREC_BOUND
    assert float(re.search(r'double\s+jrec_ratio\s*=\s*([0-9.e+-]+)', src).group(1)) == JREC_RATIO
    assert int(re.search(r'int\s+jrec_min\s*=\s*([0-9]+)', src).group(1)) == JREC_MIN
