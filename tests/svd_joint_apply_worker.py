"""Child process of tests/test_gpu_svd_joint_apply.py: the batched SVD of one named list under whatever CYB_* switches the
parent put into the environment (they are read once per process).  Every block is checked against numpy.linalg.svd with the
criteria of tests/test_gpu_decomp.py (1e-10 relative to the block norm); S of every block goes to the .npz file named on the
command line.  Prints OK or raises.

    python svd_joint_apply_worker.py <list name> <out.npz>
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-10


def product(rng, m, n, r):
    return rng.standard_normal((m, r)) @ rng.standard_normal((r, n))


def eightfold(rng, m, n, cplx=False):
    """U diag(s) V^H with s in groups of eight equal values, in no order."""
    k = min(m, n)

    def randn(shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape) if cplx else rng.standard_normal(shape)
    q1, _ = np.linalg.qr(randn((m, k)))
    q2, _ = np.linalg.qr(randn((n, k)))
    s = np.repeat(rng.random(k // 8) + 0.1, 8)
    return (q1 * rng.permutation(s)) @ q2.conj().T


def lists(name):
    """name -> (blocks, complex entry point?)"""
    rng = np.random.default_rng(2024)
    if name == 'mixed':
        # LQ blocks square / wide / tall (ranks 160 and 144: with CYB_SVD_JREC_MIN between them one recovers its rotations and
        # two accumulate them) and a full-rank block without an LQ step, which has a Q1 target only
        return [product(rng, 320, 320, 160), product(rng, 288, 416, 144), product(rng, 416, 288, 144), rng.standard_normal((160, 160))], False
    if name in ('eight', 'seven'):
        # wide targets of one application: 8 x 544 = 4352 columns (the default rule takes the wide route), 7 x 544 = 3808 (strips)
        return [product(np.random.default_rng(100 + i), 544, 544, 272) for i in range(8 if name == 'eight' else 7)], False
    if name == 'ties':
        return [eightfold(rng, 192, 192), eightfold(rng, 192, 256), eightfold(rng, 256, 192)], False
    if name == 'ties-complex':
        return [eightfold(rng, 192, 192, True), eightfold(rng, 96, 128, True), eightfold(rng, 128, 96, True)], True
    if name == 'early-stop':
        return [product(rng, 320, 320, 160), product(rng, 320, 320, 150)], False
    raise KeyError(name)


def check(a, U, S, Vh):
    k = min(a.shape)
    nrm = np.linalg.norm(a)
    sref = np.linalg.svd(a, compute_uv=False)
    figs = {'S': np.abs(S - sref).max() / nrm, 'rec': np.abs((U * S) @ Vh - a).max() / nrm,
            'U': np.abs(U.conj().T @ U - np.eye(k)).max(), 'Vh': np.abs(Vh @ Vh.conj().T - np.eye(k)).max()}
    print(a.shape, ' '.join(f'{n} {v:.2e}' for n, v in figs.items()), flush=True)
    assert U.shape == (a.shape[0], k) and S.shape == (k,) and Vh.shape == (k, a.shape[1])
    assert np.all(S >= 0) and np.all(S[:-1] >= S[1:])
    assert all(v <= TOL for v in figs.values()), figs
    # the null vectors on their own: orthonormal, and orthogonal to the vectors of the non-zero values
    r = int(np.linalg.matrix_rank(a))
    if r < k:
        for F in (U, Vh.conj().T):
            assert np.abs(F[:, r:].conj().T @ F[:, r:] - np.eye(k - r)).max() <= TOL
            assert np.abs(F[:, :r].conj().T @ F[:, r:]).max() <= TOL


def main(name, out):
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    mats, cplx = lists(name)
    print(f'[case] {name}', file=sys.stderr, flush=True)
    if cplx:
        got = bb._complex_svd_embedded(bb.contiguous_many([bb.as_block(m) for m in mats]))
        assert got is not None
        res = got[0]
    else:
        res = bb.matrix_svd_batched([bb.as_block(m) for m in mats])
    s_all = {}
    for i, (m, (U, S, Vh)) in enumerate(zip(mats, res)):
        U, S, Vh = bb.to_numpy(U), bb.to_numpy(S), bb.to_numpy(Vh)
        check(m, U, S, Vh)
        s_all[f'S{i}'] = S
    np.savez(out, **s_all)
    print('OK')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
