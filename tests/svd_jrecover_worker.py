"""Child process of tests/test_gpu_svd_jrecover.py: the batched SVD of every case of `cases()`, one block per call (so that
the route line of `CYB_SVD_TRACE_REDO` belongs to that block alone and a fallback of one block does not redo another), under
whatever CYB_SVD_* switches the parent put into the environment (they are read once per process).  Every case is checked
against LAPACK with the criteria of tests/test_gpu_fullsize.py; the singular values go to the .npz named on the command
line.  A line `[case] <name>` on stderr precedes each call.  Prints OK or raises."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = [(96, 96), (200, 200), (721, 824), (1442, 1442)]


def _orth(rng, n, k):
    q, r = np.linalg.qr(rng.standard_normal((n, k)))
    return q * np.sign(np.diag(r))


def cases():
    """name -> matrix: the families of tests/test_svd_jrecover_model.py at the four sizes, seeded."""
    out = {}
    for m, n in SIZES:
        rng = np.random.default_rng(1000 * m + n)
        k = min(m, n)
        tag = f'{m}x{n}'
        out[f'theta {tag}'] = rng.standard_normal((m, k // 2)) @ rng.standard_normal((k // 2, n)) / (k // 2) ** 0.5
        out[f'gaussian {tag}'] = rng.standard_normal((m, n))
        for d in (4, 8, 12, 14):
            out[f'spectrum {d} decades {tag}'] = (_orth(rng, m, k) * np.logspace(0, -d, k)) @ _orth(rng, n, k).T
        out[f'columns 8 decades {tag}'] = rng.standard_normal((m, n)) * np.logspace(0, -8, n)
        z = rng.standard_normal((m, n))
        if m < n:   # (the factored matrix is the tall orientation: its zero columns are the zero rows of a wide block)
            z[rng.choice(m, m // 3, replace=False), :] = 0.0
        else:
            z[:, rng.choice(n, n // 3, replace=False)] = 0.0
        out[f'zero columns {tag}'] = z
        t = out[f'theta {tag}'].copy()      # a zero column among the first: R keeps one more row than the rank
        if m < n:
            t[rng.choice(k // 8, 3, replace=False), :] = 0.0
        else:
            t[:, rng.choice(k // 8, 3, replace=False)] = 0.0
        out[f'theta, zero columns {tag}'] = t
        s = np.linspace(2.0, 1.0, k)
        s[k // 3:k // 3 + 10] = 1.5
        out[f'repeated value {tag}'] = (_orth(rng, m, k) * s) @ _orth(rng, n, k).T
    return out


def main(path):
    from helpers import check_svd_invariants
    from cyten_amd.block_backend import HipBlockBackend
    bb = HipBlockBackend('cuda:0')
    svals = {}
    for name, a in cases().items():
        sys.stderr.write(f'[case] {name}\n')
        sys.stderr.flush()
        (U, S, Vh), = bb.matrix_svd_batched([bb.as_block(a)])
        U, S, Vh = bb.to_numpy(U), bb.to_numpy(S), bb.to_numpy(Vh)
        sref = np.linalg.svd(a, compute_uv=False)
        k, nrm = min(a.shape), np.linalg.norm(a)
        print(f'{name:34s} |dS| {np.abs(S - sref).max() / nrm:.1e}  rec {np.abs((U * S) @ Vh - a).max() / nrm:.1e}  '
              f'UtU {np.abs(U.T @ U - np.eye(k)).max():.1e}  VVt {np.abs(Vh @ Vh.T - np.eye(k)).max():.1e}', flush=True)
        check_svd_invariants(a, U, S, Vh, 1e-10, sref=sref)
        svals[name] = S
    np.savez(path, **svals)
    print('OK')


if __name__ == '__main__':
    main(sys.argv[1])
