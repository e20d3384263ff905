"""Child process of tests/test_gpu_decomp_accuracy.py::test_switch_variants: the compact list of
tests/decomp_accuracy_cases.py::worker_cases -- pipeline, rotations accumulated and recovered, panels of more than 1536 rows,
embedded complex blocks, eigh on the engine -- under whatever CYB_* switches the parent put into the environment (they are read
once per process).  Every result is held to the cap of 1e-13; prints one line of measures per case, then OK, or raises."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decomp_accuracy_cases as dac   # noqa: E402
from cyten_amd.block_backend import HipBlockBackend   # noqa: E402

bb = HipBlockBackend('cuda:0')
failures = []


def held(route, case, check, *arrays, **kw):
    try:
        print(dac.table_line(route, case, check(case, *arrays, **kw)), flush=True)
    except dac.AccuracyError as e:
        print(f'[accuracy] {route}: FAILED {e}', flush=True)
        failures.append(str(e))


def svd(route, cases, caps=None):
    print(f'[list] {route}', file=sys.stderr, flush=True)          # (the engine's own route trace goes to stderr as well)
    res = bb.matrix_svd_batched([bb.as_block(c.a) for c in cases])
    for c, (U, S, Vh) in zip(cases, res):
        held(route, c, dac.check_svd, bb.to_numpy(U), bb.to_numpy(S), bb.to_numpy(Vh), caps=(caps or {}).get(c.name))


def eigh(route, cases):
    res = bb.eigh_batched([bb.as_block(c.a) for c in cases])
    for c, (W, V) in zip(cases, res):
        held(route, c, dac.check_eigh, bb.to_numpy(W), bb.to_numpy(V))


lists = dac.worker_cases()
svd('svd pipeline', [c for c in lists['svd'] if 'r0' not in c.name])
svd('svd r0', [c for c in lists['svd'] if 'r0' in c.name])
if 'CYB_JACOBI_NOSWEEP' in os.environ:
    # The one individual cap of the module ("Measured accuracy").  Without the persistent sweep kernel the engine
    # refuses embedded complex rows and the complex Jacobi kernels stand in, on a 256 x 128 block of rank 64 -- beyond the
    # min(m, n) <= 95 they are routed for.  They iterate on A itself, without a QR in front: its 64 null columns end as rounding
    # noise of norm 1.0e-13 sigma_1 (452 eps), below the kernels' own rank threshold 2.3e-16 M ||A||_F, and those norms are
    # the singular values reported for them.  `values` of that block is held to that threshold; everything else to the cap.
    c = lists['csvd'][2]
    assert c.name == 'exact rank 64 256x128'
    svd('csvd complex kernels', lists['csvd'], caps={c.name: {'values': dac.complex_jacobi_null_cap(c)}})
else:
    svd('csvd embedded', lists['csvd'])
eigh('eigh engine', lists['eigh'])
eigh('ceigh embedded', lists['ceigh'])
bb.synchronize()
if failures:
    raise SystemExit('\n'.join(['above the cap:'] + failures))
print('OK')
