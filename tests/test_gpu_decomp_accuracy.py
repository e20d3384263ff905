"""SVD, QR / LQ and eigh held to the rounding level: every measure of tests/decomp_accuracy_cases.py -- orthogonality,
residual, values against references of negligible error (an exact family, mpmath at 50 digits), all formed in long double --
must stay at or below 1e-13 (450 eps) on every route of the batched decompositions; the structural facts hold exactly.
tests/test_decomp_accuracy_model.py shows that LAPACK meets an eighth of that cap on the same cases and that the measures
catch defects of 1e-12.

Routing depends on the whole list (`svd_batched_impl`: the in-LDS kernel runs when every block fits it or at least 16 do,
otherwise every block with min(m, n) >= 2 joins the QR pipeline), so every route is driven by a list built to reach it.  The
C-ABI entry is observed with the recording proxy of tests/test_gpu_decomp_routes.py; what that cannot see (which kernel behind
one entry) follows from the shapes by the rule restated in `_fits_lds` and is named in the printed table.  Switches are read
once per process: the variants run tests/decomp_accuracy_worker.py as a child, one at a time.

Every case prints one line: route, case, shape, orth_u, orth_v, resid, values in units of eps = 2^-52."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import decomp_accuracy_cases as dac
from helpers import check_svd_accuracy
from test_gpu_decomp import test_svd_pipeline_variants as _pipeline_variants
from test_gpu_decomp_routes import RecordingLib

pytestmark = pytest.mark.gpu


@pytest.fixture
def rec(bb, monkeypatch):
    proxy = RecordingLib(bb.lib)
    monkeypatch.setattr(bb, 'lib', proxy)
    return proxy


@pytest.fixture(scope='module')
def svd_real():
    return dac.svd_real_groups()


@pytest.fixture(scope='module')
def svd_complex():
    return dac.svd_complex_groups()


@pytest.fixture(scope='module')
def eigh_cases():
    return dac.eigh_groups()


@pytest.fixture(scope='module')
def qr_complex():
    return dac.qr_complex_groups()


class Table:
    """Prints the line of every case, collects what is above the cap, fails at the end: one run shows every figure."""

    def __init__(self, route):
        self.route, self.failures = route, []

    def hold(self, case, check, *arrays, tag='', **kw):
        try:
            print(dac.table_line(self.route + tag, case, check(case, *arrays, **kw)))
        except dac.AccuracyError as e:
            print(f'[accuracy] {self.route + tag}: FAILED {e}')
            self.failures.append(str(e))

    def done(self):
        assert not self.failures, '\n'.join(self.failures)


def _fits_lds(shape):
    return min(shape) <= 64 and max(shape) <= 128      # cyb::svd_small_fits


def _svd_list(bb, table, cases):
    res = bb.matrix_svd_batched([bb.as_block(c.a) for c in cases])
    for c, (U, S, Vh) in zip(cases, res):
        table.hold(c, dac.check_svd, bb.to_numpy(U), bb.to_numpy(S), bb.to_numpy(Vh))


# ---- real SVD
def test_real_svd_in_lds(bb, rec, svd_real):
    cases = svd_real['in-LDS']
    assert all(_fits_lds(c.shape) for c in cases)
    table = Table('svd_small (in-LDS)')
    _svd_list(bb, table, cases)
    assert rec.calls('cyb_svd_') == [('cyb_svd_batched_f64', len(cases))]
    table.done()


@pytest.mark.parametrize('group', ['tiny blocks in the pipeline', 'pipeline, no deflation', 'pipeline, deflation and completion',
                                   'pipeline, early stop off a panel boundary', 'pipeline, panels of more than 1536 rows'])
def test_real_svd_pipeline(bb, rec, svd_real, group):
    cases = svd_real[group]
    fit = [c for c in cases if _fits_lds(c.shape)]
    assert len(fit) < min(16, len(cases)) and all(min(c.shape) >= 2 for c in cases)       # nothing is left to the in-LDS kernel
    if group.startswith('tiny'):
        assert len(fit) == 2
    table = Table(group)
    _svd_list(bb, table, cases)
    assert rec.calls('cyb_svd_') == [('cyb_svd_batched_f64', len(cases))]
    table.done()


def test_strict_helper_agrees_with_the_case_checks(bb, svd_real):
    """`helpers.check_svd_accuracy`, the strict sibling of `check_svd_invariants`, on a block with and without reference values."""
    c = svd_real['in-LDS'][-3]
    (U, S, Vh), = bb.matrix_svd_batched([bb.as_block(c.a)])
    U, S, Vh = bb.to_numpy(U), bb.to_numpy(S), bb.to_numpy(Vh)
    assert c.origin == 'mpmath' and check_svd_accuracy(c.a, U, S, Vh, sref=c.ref) == dac.check_svd(c, U, S, Vh)
    assert 'values' not in check_svd_accuracy(c.a, U, S, Vh)
    with pytest.raises(AssertionError):
        check_svd_accuracy(c.a, U, S * (1 + 1e-12), Vh, sref=c.ref)


# ---- complex SVD
@pytest.mark.parametrize('group', ['csvd_small', 'csvd_large', 'embedded'])
def test_complex_svd(bb, rec, svd_complex, group):
    cases = svd_complex[group]
    mins = [min(c.shape) for c in cases]
    assert all({'csvd_small': k <= 64, 'csvd_large': 65 <= k <= 95, 'embedded': k >= bb.COMPLEX_SVD_EMBED_MIN}[group] for k in mins)
    table = Table('complex svd ' + group)
    _svd_list(bb, table, cases)
    calls = rec.calls('cyb_svd_')
    if group == 'embedded':
        assert calls[0] == ('cyb_svd_batched_ex_f64', len(cases))
        handed_back = sum(n for name, n in calls[1:] if name == 'cyb_svd_batched_c128')
        print(f'[accuracy] complex svd embedded: {handed_back} of {len(cases)} blocks handed back to the complex kernels')
        assert [name for name, _ in calls[1:]] in ([], ['cyb_svd_batched_c128'])
        assert handed_back <= sum(1 for c in cases if c.rank is not None and c.rank < min(c.shape))    # full rank: never
    else:
        assert calls == [('cyb_svd_batched_c128', len(cases))]
    table.done()


# ---- eigh
@pytest.mark.parametrize('group,entry', [('real in-LDS', 'cyb_eigh_batched_f64'), ('real engine', 'cyb_eigh_batched_f64'),
                                         ('complex small', 'cyb_eigh_batched_c128'), ('complex large', 'cyb_eigh_batched_c128'),
                                         ('complex embedded', 'cyb_eigh_batched_ex_f64')])
def test_eigh(bb, rec, eigh_cases, group, entry):
    cases = eigh_cases[group]
    ns = [c.shape[0] for c in cases]
    assert all({'real in-LDS': n <= 64, 'real engine': n > 64, 'complex small': n <= 64, 'complex large': 64 < n < bb.COMPLEX_EIGH_EMBED_MIN,
                'complex embedded': n >= bb.COMPLEX_EIGH_EMBED_MIN}[group] for n in ns)
    table = Table('eigh ' + group)
    res = bb.eigh_batched([bb.as_block(c.a) for c in cases])
    assert rec.calls('cyb_eigh_') == [(entry, len(cases))]
    for c, (W, V) in zip(cases, res):
        table.hold(c, dac.check_eigh, bb.to_numpy(W), bb.to_numpy(V))
    table.done()


# ---- QR / LQ
@pytest.mark.parametrize('full', [False, True], ids=['thin', 'full'])
def test_real_qr_and_lq(bb, rec, full):
    cases = dac.qr_real_cases()
    table = Table('real qr')
    for c, (Q, R) in zip(cases, bb.matrix_qr_batched([bb.as_block(c.a) for c in cases], full)):
        table.hold(c, dac.check_qr, bb.to_numpy(Q), bb.to_numpy(R), tag=' full' if full else ' thin', full=full)
    for c, (L, Q) in zip(cases, bb.matrix_lq_batched([bb.as_block(c.a) for c in cases], full)):
        L, Q = bb.to_numpy(L), bb.to_numpy(Q)
        ct = dac.Case(c.name + ' (LQ)', np.ascontiguousarray(c.a.T))     # A = L Q  <=>  A^T = Q^T L^T
        table.hold(ct, dac.check_qr, np.ascontiguousarray(Q.T), np.ascontiguousarray(L.T), tag=' full' if full else ' thin', full=full)
    assert rec.calls('cyb_qr_') == [('cyb_qr_batched_f64', len(cases))] * 2
    table.done()


@pytest.mark.parametrize('full', [False, True], ids=['thin', 'full'])
@pytest.mark.parametrize('group', ['one-workgroup kernel', 'step kernel', 'embedded', 'embedded, rank deficient'])
def test_complex_qr(bb, rec, qr_complex, group, full):
    """Both complex routes promise diag(R) real and >= 0 (the same factorisation whichever route a block took)."""
    cases = qr_complex[group]
    blocks = [bb.as_block(c.a) for c in cases]
    if group == 'step kernel':       # the complex Householder kernels directly: working copies of more than 96 x 96 elements
        over = [c.shape[0] * max(c.shape[1], c.shape[0] if full else min(c.shape)) > 96 * 96 for c in cases]
        assert all(over) if full else any(over)      # (120 x 40 needs the step kernel only for its full Q)
        res = bb.matrix_qr_batched_direct(bb.contiguous_many(blocks), full, True)
    else:
        res = bb.matrix_qr_batched(blocks, full)
    calls = rec.calls('cyb_qr_')
    if group == 'one-workgroup kernel':
        assert all(c.shape[0] * max(c.shape) <= 96 * 96 for c in cases)
        assert calls == [('cyb_qr_batched_c128', len(cases))]
    elif group == 'step kernel':
        assert calls == [('cyb_qr_batched_c128', len(cases))]
    else:
        assert calls[0] == ('cyb_qr_batched_f64', len(cases))
        handed_back = sum(n for name, n in calls if name == 'cyb_qr_batched_c128')
        print(f'[accuracy] complex qr {group}: entries {calls}; {handed_back} blocks handed back to the complex kernels')
        if group == 'embedded':
            assert handed_back == 0 and len(calls) == 1          # full rank: structured to rounding, no second pass
    table = Table('complex qr ' + group)
    for c, (Q, R) in zip(cases, res):
        table.hold(c, dac.check_qr, bb.to_numpy(Q), bb.to_numpy(R), tag=' full' if full else ' thin', full=full, positive_diagonal=True)
    table.done()


# ---- switch variants: one child per switch
_mark = next(m for m in _pipeline_variants.pytestmark if m.name == 'parametrize')
VARIANTS = list(zip(_mark.kwargs['ids'], _mark.args[1])) + [
    ('round-passes-unfolded', {'CYB_JACOBI_ROUND_PASSES': '0'}),
    ('last-sweep-never-predicted', {'CYB_JACOBI_NOPREDICT': '1'}),
    ('recovery-from-160-rows', {'CYB_SVD_JREC_MIN': '160'}),
    ('recovery-from-160-rows-then-redone', {'CYB_SVD_JREC_MIN': '160', 'CYB_SVD_JREC_FORCE_REDO': '1'}),
    ('recovery-redo-forced', {'CYB_SVD_JREC_FORCE_REDO': '1'})]


def _traced_routes(stderr):
    """{list name: [(r0, route) per block]} from the engine's trace (CYB_SVD_TRACE_REDO), first report per list."""
    out, name = {}, None
    for line in stderr.splitlines():
        if line.startswith('[list] '):
            name = line[7:]
        m = re.match(r'\[cyb\] svd jrec: block (\d+) \(\d+ x \d+, r0 (\d+)\): ([a-zA-Z ]+) \(', line)
        if m and name is not None and int(m.group(1)) == len(out.setdefault(name, [])):
            out[name].append((int(m.group(2)), m.group(3)))
    return out


@pytest.mark.parametrize('env', [v[1] for v in VARIANTS], ids=[v[0] for v in VARIANTS])
def test_switch_variants(env):
    """The worker's list under every switch of `test_svd_pipeline_variants`, with the round's passes unfolded, without the
    predicted last sweep, and with the rotation recovery admitted from 160 rows (the blocks of r0 = 176 then recover their
    rotations, those of r0 = 144 accumulate them), redone, and forced to redo: the same cap for all of them.  The one exception
    of the module is made in the worker: under `per-round` the complex Jacobi kernels stand in for the embedded
    route on a 256 x 128 block of rank 64, and `values` of that block is held to their own rank threshold (measured 452.2 eps,
    threshold 1222 eps, cap 450.4 eps)."""
    e = dict(os.environ)
    for k in ('CYB_SVD_JREC_MIN', 'CYB_SVD_JREC_FORCE_REDO', 'CYB_SVD_NOJREC', 'CYB_SVD_JREC_RATIO'):
        e.pop(k, None)
    e.update(env)
    e['CYB_SVD_TRACE_REDO'] = '1'
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), 'decomp_accuracy_worker.py')], env=e, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-8000:])
    routes = _traced_routes(r.stderr)
    for name, blocks in routes.items():
        print(f'[accuracy] {name}: ' + ', '.join(f'r0 {r0} {route}' for r0, route in blocks))
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-3000:] + r.stderr[-4000:]
    if env.get('CYB_SVD_JREC_MIN') == '160':
        # list 'svd r0': full r0 144, graded r0 144, full r0 176, graded r0 176
        (a0, ra), _, (b0, rb), (g0, rg) = routes['svd r0']
        assert a0 < 160 <= b0 < 256 and 160 <= g0
        assert ra == 'excluded' and rg == 'excluded'
        assert rb == ('recovered then redone' if 'CYB_SVD_JREC_FORCE_REDO' in env else 'recovered')
