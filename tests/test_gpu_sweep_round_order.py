"""Issue order of a round of the persistent sweep kernel: the update's operands are prefetched behind the
Gram exchange, the Gram MFMAs follow their own loads, both counters of a hand-off are polled in flight together.  None of
that touches a sum or the protocol, so `CYB_JACOBI_ROUND_ORDER=0` (the order before) must give the SAME BITS: every group of
cases runs twice, each run in a fresh child process (the switches are read once per process), every result is checked
against numpy at 1e-10 there, and S, U and Vh (w and V of the eigh case) of the two runs are compared block by block here.

Groups and the paths they reach (tests/sweep_round_order_worker.py):
  default  theta 600x640 of rank 300 (recovered block: no J in the sweeps, ct = nW <= SW_PRE, G > 1, cross and full rounds);
           Gaussian 200x200 (no LQ step, J accumulated and deferred, the pendP path, a sweep's last round updates J at once);
           eye(128) and ones(96, 64) (skip rounds that publish without an update); symmetric 200x200 through eigh_batched (no
           J, no QR); complex 130x130 and 180x40.40x150 through the embedded route (CPLX instantiation); one call with the
           600x640, the 200x200 and twelve Gaussian blocks of 20^2 .. 90^2 (a list; small blocks run three inner sweeps)
  g2       Gaussian 900x900 with CYB_JACOBI_G=2 (nW = 7 > SW_PRE: the streaming loop behind the prefetch registers, J chunks
           loaded after the readyJ wait)
  g1       the same block with CYB_JACOBI_G=1 (no exchange: prefetch placement and LDS aliasing without the poll)
  nolq     theta 300x260 of rank 120 with CYB_SVD_NOLQ=1 (in-kernel deflation, the any_null branch)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from sweep_round_order_worker import GROUPS, cases

pytestmark = pytest.mark.gpu

SWITCHES = ('CYB_JACOBI_ROUND_ORDER', 'CYB_JACOBI_G', 'CYB_SVD_NOLQ')


def _run(group, parent_order, path):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(GROUPS[group])
    if parent_order:
        e['CYB_JACOBI_ROUND_ORDER'] = '0'
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), 'sweep_round_order_worker.py'), group, str(path)],
                       env=e, capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-3000:] + r.stderr[-4000:]
    return dict(np.load(path))


@pytest.mark.parametrize('group', list(GROUPS))
def test_round_order_keeps_every_bit(group, tmp_path):
    new = _run(group, False, tmp_path / 'new.npz')
    old = _run(group, True, tmp_path / 'old.npz')
    want = sorted(f'{name}|{i}|{j}' for name, kind, mats in cases(group) for i in range(len(mats)) for j in range(2 if kind == 'eigh' else 3))
    assert sorted(new) == want and sorted(old) == want      # nothing was left out
    for key in want:
        assert new[key].dtype == old[key].dtype and new[key].shape == old[key].shape, key
        assert np.array_equal(new[key], old[key]), key
