"""Rotation recovery of the batched SVD: blocks on the LQ branch whose R2 is well enough conditioned iterate
without accumulating the rotations J'; J' is rebuilt afterwards from S Z^T and R2, its deviation from an isometry measured on
the device, and a block above the bound (or with a numerically null row) sends the call to the plain iteration with
accumulation.  The families of tests/test_svd_jrecover_model.py at 96, 200, 721 x 824 and 1442^2 against LAPACK with the
criteria of tests/test_gpu_fullsize.py (1e-10 relative to the block norm), with the recovery on, off and with its fallback
forced -- each in a fresh child process, as the switches are read once per process."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = {'on': {}, 'off': {'CYB_SVD_NOJREC': '1'}, 'forced-redo': {'CYB_SVD_JREC_FORCE_REDO': '1'}}


def _run(mode, path):
    e = dict(os.environ)
    for k in ('CYB_SVD_NOJREC', 'CYB_SVD_JREC_FORCE_REDO', 'CYB_SVD_JREC_RATIO', 'CYB_SVD_JREC_MIN'):
        e.pop(k, None)
    e.update(MODES[mode])
    e['CYB_SVD_TRACE_REDO'] = '1'
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), 'svd_jrecover_worker.py'), str(path)], env=e,
                       capture_output=True, text=True, timeout=1500)
    print(r.stdout[-8000:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-3000:] + r.stderr[-4000:]
    routes, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith('[case] '):
            name = line[7:]
        m = re.match(r'\[cyb\] svd jrec: block 0 \(.*\): ([a-zA-Z ]+) \(deviation ([0-9.e+-]+|inf|nan),', line)
        if m:
            routes[name] = (m.group(1), float(m.group(2)))
    for n, rt in routes.items():
        print(f'{mode:12s} {n:34s} {rt[0]:22s} deviation {rt[1]:.1e}')
    return routes, dict(np.load(path))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp('jrec')
    return {mode: _run(mode, d / f'{mode}.npz') for mode in MODES}


def test_every_case_meets_the_criteria_on_every_route(runs):
    from svd_jrecover_worker import cases
    names = list(cases())
    for mode in MODES:           # (the worker asserted the criteria case by case; here: nothing was left out)
        assert sorted(runs[mode][1]) == sorted(names)
        assert sorted(runs[mode][0]) == sorted(names)   # every case went through the pipeline and reported its route


def test_all_three_routes_are_exercised(runs):
    routes = runs['on'][0]
    kinds = {r[0] for r in routes.values()}
    assert {'recovered', 'excluded', 'recovered then redone'} <= kinds, kinds
    # what the CPU model predicts: the benchmark's kind (condition of R2 ~ 10) is recovered to rounding; every graded
    # spectrum is refused up front; a theta with zero columns among its first is admitted and then found by the null-row rule
    for tag in ('721x824', '1442x1442'):
        assert routes[f'theta {tag}'][0] == 'recovered' and routes[f'theta {tag}'][1] <= 2e-12
        assert routes[f'repeated value {tag}'][0] in ('recovered', 'no LQ step')
        for d in (8, 12, 14):
            assert routes[f'spectrum {d} decades {tag}'][0] == 'excluded'
        assert routes[f'columns 8 decades {tag}'][0] in ('excluded', 'no LQ step')
        assert routes[f'theta, zero columns {tag}'][0] == 'recovered then redone'
    assert routes['theta 96x96'][0] == 'excluded'
    for n, (kind, dev) in routes.items():
        if kind == 'recovered':
            assert dev <= 2e-11, (n, dev)


def test_switches_select_the_route(runs):
    assert all(r[0] in ('excluded', 'no LQ step') for r in runs['off'][0].values())
    on, forced = runs['on'][0], runs['forced-redo'][0]
    for n in on:
        if on[n][0] == 'recovered':
            assert forced[n][0] == 'recovered then redone'


def _s_differences(runs):
    on, off = runs['on'], runs['off']
    out = {}
    for n, s in on[1].items():
        if on[0][n][0] != 'recovered then redone':
            out[n] = np.abs(s - off[1][n]).max() / s[0]
            if out[n] != 0.0:
                print(f'{n:34s} max |S_on - S_off| / S_0 = {out[n]:.2e}')
    print(f'worst relative difference of S between recovery on and off: {max(out.values()):.2e}')
    return out


def test_singular_values_agree_with_the_recovery_on_and_off(runs):
    """Parts per pair are what they were (JMat::rec_j), so the sweeps are the same with the recovery on and off; S agrees to
    1e-13 of the largest value wherever the block was not redone."""
    for n, d in _s_differences(runs).items():
        assert d <= 1e-13, (n, d)


def test_singular_values_are_bit_identical_with_the_recovery_on_and_off(runs):
    """The sweeps do not read J, and S is read off the row norms of S Z^T alone (`PostDesc::sig_lq`), not off rows that went
    through J': the same bits with the rotations accumulated or recovered, wherever the block was not redone."""
    on, off = runs['on'], runs['off']
    _s_differences(runs)
    for n, s in on[1].items():
        if on[0][n][0] != 'recovered then redone':
            assert np.array_equal(s, off[1][n]), n
