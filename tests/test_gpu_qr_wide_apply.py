"""The two routes of the application of Q (csrc/blocked_qr.hip, `bqr_apply_q`): 32-column strips panel by panel, or groups
of CYB_QR_APPLY_WIDTH reflector columns through the grouped GEMM with merged T factors.  Both apply the same orthogonal
matrix: every setting is checked against LAPACK, and the settings against each other -- R and S bit for bit (they never pass
through the application), Q / U / Vh to 1e-12 sqrt(k), the rounding bound of tests/test_qr_wide_merge_model.py with margin.
The default setting must give byte for byte what the forced setting of its shape rule gives.  The switches are read once per
process, hence one child process per setting (qr_wide_apply_worker.py)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.linalg

from helpers import check_svd_invariants
from qr_wide_apply_worker import inputs

pytestmark = pytest.mark.gpu
TOL = 1e-10
SETTINGS = {'strips': {'CYB_QR_APPLY_WIDE': '0'}, 'wide128': {'CYB_QR_APPLY_WIDE': '1', 'CYB_QR_APPLY_WIDTH': '128'},
            'wide64': {'CYB_QR_APPLY_WIDE': '1', 'CYB_QR_APPLY_WIDTH': '64'}, 'default': {}}
# the shape rule of blocked_qr.hip (`wide_target`, `bqr_apply_q`): reflector columns of the matrix, columns of the target, and
# the columns of all such targets of the call together
WIDE_MIN_K, WIDE_MIN_KC, WIDE_MIN_COLS = 256, 256, 4096


def _call_routes(targets):
    """The forced setting the default rule selects for every (k, kc) target of ONE call of the application of Q."""
    cand = [k > 32 and k >= WIDE_MIN_K and kc >= WIDE_MIN_KC for k, kc in targets]
    cols = sum(kc for (k, kc), c in zip(targets, cand) if c)
    return ['wide128' if c and cols >= WIDE_MIN_COLS else 'strips' for c in cand]


def _routes(kind, full, mats):
    """Per matrix of the input: the set of forced settings the default rule selects for the applications of Q it goes through."""
    shapes = [(2 * a.shape[0], 2 * a.shape[1]) if np.iscomplexobj(a) else a.shape for a in mats]
    if kind == 'qr':
        idx = [i for i, (m, n) in enumerate(shapes) if min(m, n) >= 96]     # (smaller blocks: the unblocked kernel)
        out = [set() for _ in mats]
        for i, r in zip(idx, _call_routes([(min(shapes[i]), shapes[i][0] if full else min(shapes[i])) for i in idx])):
            out[i] = {r}
        return out
    # SVD: Q1 (k reflector columns, applied to k columns) and Q2 of the LQ step (rank reflector columns, k columns), one call each
    ks = [min(s) for s in shapes]
    r0 = [np.linalg.matrix_rank(a) * (2 if np.iscomplexobj(a) else 1) for a in mats]
    q1, q2 = _call_routes([(k, k) for k in ks]), _call_routes(list(zip(r0, ks)))
    return [{x, y} for x, y in zip(q1, q2)]


@pytest.fixture(scope='module')
def runs():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, env in SETTINGS.items():
            d = os.path.join(tmp, name)
            os.mkdir(d)
            e = {k: v for k, v in os.environ.items() if not k.startswith('CYB_QR_APPLY_')}
            e.update(env)
            r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), 'qr_wide_apply_worker.py'), d], env=e,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and r.stdout.strip().endswith('OK'), name + ': ' + r.stdout[-2000:] + r.stderr[-4000:]
            out[name] = {}
            for inp in inputs():
                with np.load(os.path.join(d, inp + '.npz')) as z:
                    out[name][inp] = {key: z[key] for key in z.files}
    return out


@pytest.mark.parametrize('setting', list(SETTINGS))
def test_every_setting_against_lapack(runs, setting):
    for name, (kind, full, mats) in inputs().items():
        got = runs[setting][name]
        for i, a in enumerate(mats):
            if kind == 'qr':
                Q, R = got[f'm{i}_0'], got[f'm{i}_1']
                qref, rref = scipy.linalg.qr(a, mode='full' if full else 'economic')
                assert Q.shape == qref.shape and R.shape == rref.shape, name
                assert np.abs(Q.conj().T @ Q - np.eye(Q.shape[1])).max() <= TOL, name
                assert np.abs(Q @ R - a).max() / np.linalg.norm(a) <= TOL, name
                assert np.abs(np.tril(R, -1)).max() == 0.0, name
                if not np.iscomplexobj(a):   # the same Householder sign convention as LAPACK dgeqrf: R agrees entry-wise
                    assert np.abs(R - rref).max() <= TOL * np.abs(a).max() * max(a.shape), name
                else:                        # (complex: the phases of the rows of R are a convention)
                    assert np.abs(np.abs(R) - np.abs(rref)).max() <= TOL * np.abs(a).max() * max(a.shape), name
            else:
                U, S, Vh = got[f'm{i}_0'], got[f'm{i}_1'], got[f'm{i}_2']
                sref = np.linalg.svd(a, compute_uv=False)
                if np.iscomplexobj(a):
                    k, nrm = min(a.shape), np.linalg.norm(a)
                    assert np.all(S[:-1] >= S[1:]) and np.abs(S - sref).max() <= TOL * nrm, name
                    assert np.abs((U * S) @ Vh - a).max() <= TOL * nrm, name
                    assert np.abs(U.conj().T @ U - np.eye(k)).max() <= TOL and np.abs(Vh @ Vh.conj().T - np.eye(k)).max() <= TOL, name
                else:
                    check_svd_invariants(a, U, S, Vh, TOL, sref=sref)


@pytest.mark.parametrize('setting', ['wide128', 'wide64', 'default'])
def test_settings_agree(runs, setting):
    """R and S bit for bit, Q / U / Vh to 1e-12 sqrt(k) with the strips."""
    worst = 0.0
    for name, (kind, full, mats) in inputs().items():
        got, ref = runs[setting][name], runs['strips'][name]
        for i, a in enumerate(mats):
            k = min(a.shape)
            exact = [1] if kind == 'qr' else [1]           # R of a QR, S of an SVD
            close = [0] if kind == 'qr' else [0, 2]
            for j in exact:
                assert np.array_equal(got[f'm{i}_{j}'], ref[f'm{i}_{j}']), f'{name}[{i}]: R / S differs between the routes'
            for j in close:
                diff = np.abs(got[f'm{i}_{j}'] - ref[f'm{i}_{j}']).max()
                worst = max(worst, diff / np.sqrt(k))
                print(f'{setting} {name}[{i}] factor {j}: max difference {diff:.2e} (k = {k})')
                assert diff <= 1e-12 * np.sqrt(k), f'{name}[{i}] factor {j}'
    print(f'{setting}: largest difference / sqrt(k) = {worst:.2e}')


def test_default_is_the_route_of_its_shape_rule(runs):
    """Byte for byte: the rule looks at shapes only.  (An SVD whose applications fall on both sides of the rule equals
    neither forced run; test_settings_agree bounds it.)"""
    n_checked = 0
    for name, (kind, full, mats) in inputs().items():
        for i, routes in enumerate(_routes(kind, full, mats)):
            if len(routes) != 1:
                continue
            want = runs[routes.pop()][name]
            for key, val in runs['default'][name].items():
                if key.startswith(f'm{i}_'):
                    assert val.tobytes() == want[key].tobytes(), f'{name} {key}'
                    n_checked += 1
    assert n_checked >= 60
