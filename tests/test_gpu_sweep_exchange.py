"""Exchange of the partial Grams in the persistent sweep kernel: by default they travel as tagged granules
(the data is the flag: no drain, ticket or separate poll), `CYB_JACOBI_EXCHANGE=0` selects the ticket protocol.  Both sum
the same partials in the same order, so they must give the SAME BITS: every group of cases runs twice, each run in a fresh
child process (the switches are read once per process), every result is checked against numpy at 1e-10 there, and S, U and
Vh (w and V of the eigh case) of the two runs are compared block by block here.

Groups and the paths they reach (tests/sweep_exchange_worker.py):
  default    theta 600x640 of rank 300 (recovered block: no J in the sweeps, G > 1, cross and full rounds); Gaussian 200x200
             (J accumulated and deferred: the pendP branch between the granule stores and the first sweep of them); eye(128)
             and ones(96, 64) (skip rounds); symmetric 200x200 through eigh_batched; complex 130x130 through the embedded
             route (CPLX instantiation); one call with the 600x640, the 200x200 and twelve Gaussian blocks of 20^2 .. 90^2
             (parts differ per matrix: the layout of the granule regions)
  g2, g8     Gaussian 900x900 with CYB_JACOBI_G=2 and 8 (8 = RGMAX: two groups of four parts in flight)
  g1         the same block with CYB_JACOBI_G=1 (no exchange: the new code is not reached, the LDS aliasing undisturbed)
  onelaunch  Gaussian 200x200 and 130x130 in one call with CYB_JACOBI_ONELAUNCH=1 (tags run on across the sweeps of a launch)
  nolq       theta 300x260 of rank 120 with CYB_SVD_NOLQ=1 (in-kernel deflation, any_null rounds)
  twice      the 600x640 call, a 200x200 call, the 600x640 call again in ONE process: the second result equals the first bit
             for bit (checked in the child), i.e. the tags an earlier launch left behind are gone"""
import os
import subprocess
import sys

import numpy as np
import pytest

from sweep_exchange_worker import GROUPS, cases

pytestmark = pytest.mark.gpu

SWITCHES = ('CYB_JACOBI_EXCHANGE', 'CYB_JACOBI_ROUND_ORDER', 'CYB_JACOBI_G', 'CYB_JACOBI_ONELAUNCH', 'CYB_SVD_NOLQ')


def _run(group, ticket_form, path):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(GROUPS[group])
    if ticket_form:
        e['CYB_JACOBI_EXCHANGE'] = '0'
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), 'sweep_exchange_worker.py'), group, str(path)],
                       env=e, capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-3000:] + r.stderr[-4000:]
    return dict(np.load(path))


@pytest.mark.parametrize('group', list(GROUPS))
def test_exchange_keeps_every_bit(group, tmp_path):
    new = _run(group, False, tmp_path / 'granules.npz')
    old = _run(group, True, tmp_path / 'tickets.npz')
    want = sorted(f'{name}|{i}|{j}' for name, kind, mats in cases(group) for i in range(len(mats)) for j in range(2 if kind == 'eigh' else 3))
    assert sorted(new) == want and sorted(old) == want      # nothing was left out
    for key in want:
        assert new[key].dtype == old[key].dtype and new[key].shape == old[key].shape, key
        assert np.array_equal(new[key], old[key]), key
