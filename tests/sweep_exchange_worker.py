"""Child process of tests/test_gpu_sweep_exchange.py: the cases of one group through the batched decompositions, under
whatever CYB_JACOBI_* / CYB_SVD_* switches the parent put into the environment (they are read once per process).  Every
result is checked against numpy (`helpers.check_svd_invariants` at 1e-10, as tests/sweep_round_order_worker.py does); every
factor of every block goes to the .npz named on the command line, so that the parent can compare two runs bit by bit.
Usage: sweep_exchange_worker.py <group> <out.npz>.  Prints OK or raises."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# group -> switches the parent sets for both runs of the group
GROUPS = {'default': {}, 'g2': {'CYB_JACOBI_G': '2'}, 'g8': {'CYB_JACOBI_G': '8'}, 'g1': {'CYB_JACOBI_G': '1'},
          'onelaunch': {'CYB_JACOBI_ONELAUNCH': '1'}, 'nolq': {'CYB_SVD_NOLQ': '1'}, 'twice': {}}
TOL = 1e-10


def _theta(rng, m, r, n):
    return rng.standard_normal((m, r)) @ rng.standard_normal((r, n))


def _crandn(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def cases(group):
    """[(name, kind, [matrices])], seeded; one call per entry, in this order.  kind: 'svd' | 'eigh' | 'csvd'."""
    rng = np.random.default_rng(20240923)
    theta, gauss = _theta(rng, 600, 300, 640), rng.standard_normal((200, 200))
    if group == 'default':
        sym = rng.standard_normal((200, 200))
        small = [rng.standard_normal((n, n)) for n in (20, 27, 33, 40, 46, 52, 59, 65, 72, 78, 84, 90)]
        return [('theta 600x640 rank 300', 'svd', [theta]),
                ('gaussian 200x200', 'svd', [gauss]),
                ('eye 128', 'svd', [np.eye(128)]),
                ('ones 96x64', 'svd', [np.ones((96, 64))]),
                ('symmetric 200x200', 'eigh', [sym + sym.T]),
                ('complex 130x130', 'csvd', [_crandn(rng, (130, 130))]),
                ('list', 'svd', [theta, gauss] + small)]
    if group in ('g2', 'g8', 'g1'):
        return [('gaussian 900x900', 'svd', [rng.standard_normal((900, 900))])]
    if group == 'onelaunch':
        return [('gaussian 200x200, 130x130', 'svd', [gauss, rng.standard_normal((130, 130))])]
    if group == 'nolq':
        return [('theta 300x260 rank 120', 'svd', [_theta(rng, 300, 120, 260)])]
    if group == 'twice':
        return [('theta first', 'svd', [theta]), ('gaussian between', 'svd', [gauss]), ('theta again', 'svd', [theta])]
    raise ValueError(group)


def main(group, path):
    from helpers import check_svd_invariants
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    out = {}
    for name, kind, mats in cases(group):
        blocks = [bb.as_block(m) for m in mats]
        if kind == 'svd':
            res = bb.matrix_svd_batched(blocks)
        elif kind == 'csvd':
            got = bb._complex_svd_embedded(bb.contiguous_many(blocks))
            assert got is not None, 'the embedded complex route was refused'
            res = got[0]
        else:
            res = bb.eigh_batched(blocks)
        assert len(res) == len(mats)
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
        print(f'{name}: {len(mats)} block(s) checked', flush=True)
    if group == 'twice':  # what the first launches left in the tagged words must be gone: the same call gives the same bits
        for j in range(3):
            a, b = out[f'theta first|0|{j}'], out[f'theta again|0|{j}']
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f'second call differs from the first in factor {j}'
    np.savez(path, **out)
    print('OK')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
