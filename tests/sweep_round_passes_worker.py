"""Child process of tests/test_gpu_sweep_round_passes.py: the cases of one group through the batched decompositions, under
whatever CYB_JACOBI_* / CYB_SVD_* switches the parent put into the environment (they are read once per process).  Every
result is checked against numpy at 1e-10 (`helpers.check_svd_invariants`, as tests/sweep_exchange_worker.py does); every
factor of every block AND its sweep count go to the .npz named on the command line, so that the parent can compare two runs
bit by bit.  Usage: sweep_round_passes_worker.py <group> <out.npz>.  Prints OK or raises."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sweep_exchange_worker as xw  # noqa: E402  (the shapes of that test reach the same paths; its cases are reused as they are)

# group -> switches the parent sets for both runs of the group
GROUPS = {'rounds': {}, 'clusters': {}, 'list': {}, 'nolq': {'CYB_SVD_NOLQ': '1'}, 'g1': {'CYB_JACOBI_G': '1'},
          'g2': {'CYB_JACOBI_G': '2'}, 'g8': {'CYB_JACOBI_G': '8'}, 'onelaunch': {'CYB_JACOBI_ONELAUNCH': '1'}, 'twice': {}}
TOL = 1e-10


def _eightfold(rng, n):
    """orthogonal x diag x orthogonal with every singular value eight times (the thr2 rule, near-ties in the rank)"""
    q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
    q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.repeat(np.linspace(3.0, 0.5, n // 8), 8)
    return (q1 * s) @ q2


def cases(group):
    """[(name, kind, [matrices])], seeded; one call per entry, in this order.  kind: 'svd' | 'eigh' | 'csvd'."""
    if group in ('rounds', 'clusters', 'list'):
        base = {name: (name, kind, mats) for name, kind, mats in xw.cases('default')}
        if group == 'rounds':   # cross and full rounds on a recovered block; J accumulated and deferred; eigh; CPLX
            return [base[k] for k in ('theta 600x640 rank 300', 'gaussian 200x200', 'symmetric 200x200', 'complex 130x130')]
        if group == 'clusters':  # skip rounds; only the tie rule orders perm (eye); eight-fold values
            rng = np.random.default_rng(20250611)
            return [base['eye 128'], base['ones 96x64'], ('eightfold 128x128', 'svd', [_eightfold(rng, 128)])]
        return [base['list']]   # several entries per workgroup, parts differ per matrix, full solves with three inner sweeps
    return xw.cases(group)      # nolq, g1, g2, g8, onelaunch, twice: as there


def main(group, path):
    from helpers import check_svd_invariants
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    out = {}
    for name, kind, mats in cases(group):
        blocks = [bb.as_block(m) for m in mats]
        if kind == 'svd':
            res, info = bb.matrix_svd_batched(blocks, return_info=True)
        elif kind == 'csvd':
            got = bb._complex_svd_embedded(bb.contiguous_many(blocks), True)
            assert got is not None, 'the embedded complex route was refused'
            res, info = got[0], got[1]
        else:
            res, info = bb.eigh_batched(blocks, return_info=True)
        assert len(res) == len(mats) and len(info) == len(mats)
        for i, (m, fac) in enumerate(zip(mats, res)):
            fac = [bb.to_numpy(x) for x in fac]
            nrm, k = np.linalg.norm(m), min(m.shape)
            if kind == 'svd':
                U, S, Vh = fac
                check_svd_invariants(m, U, S, Vh, TOL, sref=np.linalg.svd(m, compute_uv=False))
            elif kind == 'csvd':
                U, S, Vh = fac
                assert U.dtype == np.complex128 and S.dtype == np.float64 and np.all(S[:-1] >= S[1:])
                assert np.abs((U * S) @ Vh - m).max() <= TOL * nrm
                assert np.abs(U.conj().T @ U - np.eye(k)).max() <= TOL and np.abs(Vh @ Vh.conj().T - np.eye(k)).max() <= TOL
                assert np.abs(S - np.linalg.svd(m, compute_uv=False)).max() <= TOL * nrm
            else:
                w, V = fac
                assert np.abs(w - np.linalg.eigvalsh(m)).max() <= TOL * nrm
                assert np.abs(m @ V - V * w).max() <= TOL * nrm
                assert np.abs(V.T @ V - np.eye(k)).max() <= TOL
            for j, x in enumerate(fac):
                out[f'{name}|{i}|{j}'] = x
            assert int(info[i]) >= 0, f'{name}: block {i} reports {info[i]} sweeps'
            out[f'{name}|{i}|sweeps'] = np.int64(info[i])
        print(f'{name}: {len(mats)} block(s) checked, sweeps {[int(x) for x in info]}', flush=True)
    if group == 'twice':  # nothing in LDS or scratch survives a launch: the same call gives the same bits
        for j in (0, 1, 2, 'sweeps'):
            a, b = out[f'theta first|0|{j}'], out[f'theta again|0|{j}']
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f'second call differs from the first in {j}'
    np.savez(path, **out)
    print('OK')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
