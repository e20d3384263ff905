"""Child process of tests/test_gpu_qr_wide_apply.py: the QR / SVD inputs of that test under whatever CYB_QR_APPLY_* switches
the parent put into the environment (they are read once per process).  Writes every factor to <argv[1]>/<name>.npz and
prints OK."""
import os
import sys

import numpy as np



def inputs():
    """name -> (kind, full, list of matrices); one call of the backend per entry."""
    rng = np.random.default_rng(20)

    def crandn(shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    dep = rng.standard_normal((150, 100))
    dep[:, :40] = dep[:, 40:80] @ rng.standard_normal((40, 40))
    a200 = rng.standard_normal((200, 136))
    return {
        'qr_200x136': ('qr', False, [a200]),                     # four full panels + an 8-column one: a full and a ragged group
        'qr_200x136_full': ('qr', True, [a200]),
        'qr_260x257': ('qr', False, [rng.standard_normal((260, 257))]),   # groups of 128, 128 and 1
        'qr_96x40': ('qr', False, [rng.standard_normal((96, 40))]),       # one group narrower than W
        'qr_130x100': ('qr', False, [rng.standard_normal((130, 100))]),   # ... on the blocked path (min(m, n) >= 96)
        'qr_batch': ('qr', False, [rng.standard_normal(s) for s in [(333, 200), (96, 40), (129, 129), (700, 64), (40, 30)]]),
        # both sides of the default shape rule: sixteen targets of 257 columns (4112 together) take the wide route, the last the strips
        'qr_batch_rule': ('qr', False, [rng.standard_normal(s) for s in [(260, 257)] * 16 + [(130, 100)]]),
        'qr_1700x160': ('qr', False, [rng.standard_normal((1700, 160))]),  # panels on several workgroups, > 1536 rows under a group
        'svd_160_rank70': ('svd', None, [rng.standard_normal((160, 70)) @ rng.standard_normal((70, 160))]),
        'svd_150x100_dep': ('svd', None, [dep]),
        'svd_theta_300': ('svd', None, [rng.standard_normal((300, 120)) @ rng.standard_normal((120, 260))]),
        'svd_theta_600': ('svd', None, [rng.standard_normal((600, 280)) @ rng.standard_normal((280, 560))]),   # r0 >= 256: rotation recovery
        'cqr_130x70': ('qr', False, [crandn((130, 70))]),
        'csvd_90': ('csvd', None, [crandn((90, 89)) @ crandn((89, 90))]),
    }


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cyten_amd.block_backend import HipBlockBackend
    out = sys.argv[1]
    bb = HipBlockBackend('cuda:0')
    for name, (kind, full, mats) in inputs().items():
        blocks = [bb.as_block(m) for m in mats]
        if kind == 'qr':
            res = bb.matrix_qr_batched(blocks, full)
        elif kind == 'svd':
            res = bb.matrix_svd_batched(blocks)
        else:
            res = bb._complex_svd_embedded(bb.contiguous_many(blocks))[0]
        arrs = {}
        for i, r in enumerate(res):
            for j, x in enumerate(r):
                arrs[f'm{i}_{j}'] = bb.to_numpy(x)
        np.savez(os.path.join(out, name + '.npz'), **arrs)
    print('OK')
