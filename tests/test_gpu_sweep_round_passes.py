"""LDS passes around the pivot solve of the persistent sweep kernel: by default the round measures the
Gram from registers in one interval between two barriers, writes a cross candidate's Gram straight into interleaved
positions, ranks the rows on four waves and reads the update's operands from V through perm;
`CYB_JACOBI_ROUND_PASSES=0` selects the passes and barriers the round had before.  Both form the same terms, the same
permutation and the same operands, so they must give the SAME BITS and the same sweep counts: every group of cases runs
twice, each run in a fresh child process (the switches are read once per process), every result is checked against numpy
at 1e-10 there, and S, U, Vh (w and V of the eigh case) and the sweep count of every block of the two runs are compared here.

Groups and the paths they reach (tests/sweep_round_passes_worker.py):
  rounds     theta 600x640 of rank 300 (recovered block: no J in the sweeps, no copy of Qm, G > 1, cross and full rounds);
             Gaussian 200x200 (J accumulated and deferred: Qm copied behind the update, read by the next round's deferred
             update); symmetric 200x200 through eigh_batched; complex 130x130 through the embedded route (CPLX
             instantiation: shared prelude, wave-0 solve)
  clusters   eye(128) and ones(96, 64) (skip rounds; all keys of eye are equal: only the tie rule orders perm); 128x128
             with eight-fold singular values (the thr2 rule, near-ties in the rank)
  list       one call with the 600x640, the 200x200 and twelve Gaussian blocks of 20^2 .. 90^2 (several entries per
             workgroup, parts differ per matrix, full solves with three inner sweeps on the small ones)
  nolq       theta 300x260 of rank 120 with CYB_SVD_NOLQ=1 (null rows: the fallback path of the prelude)
  g1, g2, g8 Gaussian 900x900 with CYB_JACOBI_G=1 (no exchange in front of the measuring interval), 2 and 8 (two groups of parts)
  onelaunch  Gaussian 200x200 and 130x130 in one call with CYB_JACOBI_ONELAUNCH=1
  twice      the 600x640 call, a 200x200 call, the 600x640 call again in ONE process: the third result equals the first bit
             for bit (checked in the child), i.e. nothing in LDS or scratch survives a launch"""
import os
import subprocess
import sys

import numpy as np
import pytest

from sweep_round_passes_worker import GROUPS, cases

pytestmark = pytest.mark.gpu

SWITCHES = ('CYB_JACOBI_ROUND_PASSES', 'CYB_JACOBI_EXCHANGE', 'CYB_JACOBI_ROUND_ORDER', 'CYB_JACOBI_G', 'CYB_JACOBI_ONELAUNCH', 'CYB_SVD_NOLQ')


def _run(group, old_passes, path):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(GROUPS[group])
    if old_passes:
        e['CYB_JACOBI_ROUND_PASSES'] = '0'
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), 'sweep_round_passes_worker.py'), group, str(path)],
                       env=e, capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-3000:] + r.stderr[-4000:]
    return dict(np.load(path))


@pytest.mark.parametrize('group', list(GROUPS))
def test_round_passes_keep_every_bit(group, tmp_path):
    new = _run(group, False, tmp_path / 'folded.npz')
    old = _run(group, True, tmp_path / 'before.npz')
    want = sorted(f'{name}|{i}|{j}' for name, kind, mats in cases(group) for i in range(len(mats))
                  for j in (list(range(2 if kind == 'eigh' else 3)) + ['sweeps']))
    assert sorted(new) == want and sorted(old) == want      # nothing was left out
    for key in want:
        assert new[key].dtype == old[key].dtype and new[key].shape == old[key].shape, key
        assert np.array_equal(new[key], old[key]), key
