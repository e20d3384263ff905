"""The tail of the batched SVD: Q1 is applied to the UNSORTED J side in the same call that applies Q2 to
the LQ blocks (`bqr_apply_q_pair`), and the descending order of S is imposed where U / Vh are written out (`PostDesc::inv`,
`XposeDesc::idx`).  Every list is checked block by block against numpy.linalg.svd by tests/svd_joint_apply_worker.py, with the
1e-10 bounds of tests/test_gpu_decomp.py on S, the reconstruction and the isometry of U and Vh, S descending.  The switches
are read once per process: every run is a fresh child process, one GPU process at a time.

The 'mixed' list runs with CYB_SVD_JREC_MIN=150: its LQ blocks have ranks 160 and 144, so one recovers its rotations and two
accumulate them (the default threshold of 256 would make all three accumulate and leave the recovery out of the joint call)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ('CYB_QR_APPLY_WIDE', 'CYB_QR_APPLY_WIDTH', 'CYB_SVD_NOJREC', 'CYB_SVD_JREC_FORCE_REDO', 'CYB_SVD_LQ_FORCE_REDO',
            'CYB_SVD_JREC_RATIO', 'CYB_SVD_JREC_MIN', 'CYB_SVD_TRACE_REDO', 'CYB_SVD_NOLQ', 'CYB_SVD_LQ_ALWAYS', 'CYB_QR_TRACE_ROUTE')
MIXED = {'CYB_SVD_JREC_MIN': '150'}
WIDE = {'CYB_QR_APPLY_WIDE': '1'}
_cache = {}


def run(tmp_path_factory, name, env):
    """(S of every block, stderr) of list `name` under `env`; a run shared by two tests is made once."""
    key = (name, tuple(sorted(env.items())))
    if key not in _cache:
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        e['CYB_SVD_TRACE_REDO'] = '1'
        e['CYB_QR_TRACE_ROUTE'] = '1'
        out = tmp_path_factory.mktemp('joint') / 's.npz'
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), 'svd_joint_apply_worker.py'), name, str(out)], env=e,
                           capture_output=True, text=True, timeout=600)
        print(r.stdout[-4000:])
        assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-3000:] + r.stderr[-4000:]
        _cache[key] = (dict(np.load(out)), r.stderr)
    return _cache[key]


@pytest.mark.parametrize('route', ['1', '0'], ids=['wide-forced', 'strips-forced'])
def test_mixed_list_on_both_routes(tmp_path_factory, route):
    """LQ blocks tall / wide / square, rotations recovered (r0 = 160) and accumulated (144), and a block without an LQ step
    (a Q1 target only: the joint call is a mixed list); both targets of every block on the wide route, then on strips."""
    _, err = run(tmp_path_factory, 'mixed', {**MIXED, 'CYB_QR_APPLY_WIDE': route})
    assert 'block 0 (320 x 320, r0 160): recovered (' in err, err[-2000:]
    assert 'block 1 (288 x 416, r0 144): excluded' in err and 'block 2 (416 x 288, r0 144): excluded' in err
    assert 'block 3 (160 x 160, r0 160): no LQ step' in err


@pytest.mark.parametrize('name', ['eight', 'seven'])
def test_default_rule_on_both_sides_of_its_column_sum(tmp_path_factory, name):
    """Eight 544^2 blocks of rank 272: the wide targets of ONE application sum to 4352 >= 4096 columns and the default rule
    takes the wide route for Q1 and for Q2; seven (3808 columns) stay on strips although the joint list holds 7616.  The
    route of each of the two applications is read off the trace line of `split_routes` (CYB_QR_TRACE_ROUTE)."""
    _, err = run(tmp_path_factory, name, {})
    lines = [ln for ln in err.splitlines() if ln.startswith('[cyb] apply_q:')]
    want = ('[cyb] apply_q: 8 targets, 8 wide (4352 columns qualify), 0 on strips' if name == 'eight' else
            '[cyb] apply_q: 7 targets, 0 wide (3808 columns qualify), 7 on strips')
    assert lines == [want, want], lines


@pytest.mark.parametrize('env', [{}, WIDE], ids=['default', 'wide-forced'])
@pytest.mark.parametrize('name', ['ties', 'ties-complex'])
def test_order_is_imposed_at_write_out(tmp_path_factory, name, env):
    """Singular values in groups of eight equal ones, in no order: square, wide and tall, real and as embedded complex blocks
    (rows ranked in pairs).  U, S and Vh pair up -- the reconstruction -- and S is descending."""
    run(tmp_path_factory, name, env)


@pytest.mark.parametrize('route', ['1', '0'], ids=['wide-forced', 'strips-forced'])
@pytest.mark.parametrize('switch', ['CYB_SVD_LQ_FORCE_REDO', 'CYB_SVD_JREC_FORCE_REDO'])
def test_fallback_after_the_first_application_rebuilds_cq(tmp_path_factory, switch, route):
    """The plain iteration after the LQ one: the first pass has applied Q1 to Cq already, the second must rebuild all of it."""
    _, err = run(tmp_path_factory, 'mixed', {**MIXED, 'CYB_QR_APPLY_WIDE': route, switch: '1'})
    assert '[cyb] svd: plain iteration after the LQ one' in err, err[-2000:]
    if switch == 'CYB_SVD_JREC_FORCE_REDO':
        assert 'recovered then redone' in err


@pytest.mark.parametrize('env', [{}, WIDE], ids=['default', 'wide-forced'])
def test_early_stop_off_a_panel_boundary(tmp_path_factory, env):
    """320^2 of rank 160 and of rank 150 (off a panel boundary): the first QR stops before its last panel, Q1 has fewer
    panels than the matrix; the null vectors are orthonormal and orthogonal to the others (checked in the worker)."""
    run(tmp_path_factory, 'early-stop', env)


def test_s_is_bit_identical_with_the_rotations_recovered_or_accumulated(tmp_path_factory):
    """The guarantee of tests/test_gpu_svd_jrecover.py through the new order of the tail."""
    on, _ = run(tmp_path_factory, 'mixed', {**MIXED, **WIDE})
    off, err = run(tmp_path_factory, 'mixed', {**MIXED, **WIDE, 'CYB_SVD_NOJREC': '1'})
    assert 'recovered' not in err
    assert sorted(on) == sorted(off) == ['S0', 'S1', 'S2', 'S3']
    for k in on:
        assert np.array_equal(on[k], off[k]), k
