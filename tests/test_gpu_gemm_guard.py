"""The grouped fp64 GEMM at the C ABI on guard-band cases (tests/gemm_guard_cases.py): exact data compared bit for bit,
NaN around every operand view and inside C when beta == 0, sentinels around C, every planner branch reached on purpose.
tests/test_gemm_guard_model.py shows on the host that each kind of fault is flagged."""
import functools
import os
import subprocess
import sys

import pytest

import gemm_guard_cases as gc
from gemm_guard_worker import ENTRIES, run_case, twice_refs

pytestmark = pytest.mark.gpu

LAYOUTS = list(gc.LAYOUTS)


@functools.lru_cache(maxsize=2)
def _case(group, *args):
    """Cases are immutable (a run uploads copies of the arenas), so both entry points share one build."""
    return gc.build_case(getattr(gc, group + '_specs')(*args), 11)


def _assert_clean(bb, case, entry, runs=1, refs=None, info=None):
    rep = gc.check(case, run_case(bb, case, entry, runs, info), refs)
    assert rep.clean, str(rep)
    return rep


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_small_classes(bb, layout, entry):
    """Classes 3, 2, 5, 6, 7, 8 and the demoted class 1 with its ragged remainders in ONE call: K of one double, partial and
    full k-tiles, lists whose layout changes from segment to segment, a K = 0 segment, empty segment ranges; alpha and beta
    through {1, -2, 0.5, 0}."""
    _assert_clean(bb, _case('small_class', layout), entry)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('beta', [0.0, 1.0])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_class0_and_its_strips(bb, layout, beta, entry):
    """A filler with one 128 x 128 tile per CU keeps the call in class 0: the pointer-increment loop and every strip cut
    from a ragged edge, element by element."""
    case = _case('class0', bb.ctx.n_cu, layout, beta)
    info = {}
    _assert_clean(bb, case, entry, info=info)
    if entry == 'plan':
        # the ragged tiling of a call that KEEPS class 0: full 128-tiles plus one strip per direction with a remainder
        # (a call demoted to 64 x 64 would have more than four times the filler's tiles); a tail split, if the list is
        # longer than one round of 2 n_cu slots, adds at most one piece per tile of the last round
        n_cu = bb.ctx.n_cu
        expected = sum(-(-p.spec.M // 128) * -(-p.spec.N // 128) for p in case.probs)
        filler = case.probs[0].spec
        assert (filler.M // 128) * (filler.N // 128) >= n_cu and info['n_launches'] == 1
        assert expected <= info['n_tiles'] <= expected + 2 * n_cu
        if expected <= 2 * n_cu:
            assert info['n_tiles'] == expected


@pytest.mark.parametrize('entry', ENTRIES)
def test_degenerate_extents_in_the_tile_loader(bb, entry):
    """Extents 1 and 2: the scalar fallback of `load_tile` and its `MN - 2` clamp at an extent of exactly 2 (classes 3, 5, 6;
    the gate of the pointer-increment loop is out of reach of these entry points, see gemm_guard_cases.degenerate_specs)."""
    _assert_clean(bb, _case('degenerate'), entry)


@pytest.mark.parametrize('entry', ENTRIES)
def test_more_tiles_than_slots_and_a_plan_run_twice(bb, entry):
    """2 n_cu + 37 tiles: the persistent grid draws the rest from the atomic queue.  Run twice with beta = 1 the result is
    exactly C0 + 2 A B only if every tile ran exactly once per run, i.e. the queue heads were rewound."""
    case = _case('many_tiles', bb.ctx.n_cu)
    info = {}
    _assert_clean(bb, case, entry, runs=2, refs=twice_refs(case), info=info)
    if entry == 'plan':
        assert info['n_tiles'] == 2 * bb.ctx.n_cu + 37


@pytest.mark.parametrize('entry', ENTRIES)
def test_tail_split(bb, entry):
    """One problem with a short last queue round: its class-0 tiles are cut into 128 x 64 halves (beta = 1: a piece
    enqueued twice, or a half dropped, shows)."""
    case = _case('tail_split', bb.ctx.n_cu)
    info = {}
    _assert_clean(bb, case, entry, info=info)
    if entry == 'plan':
        sp = case.probs[0].spec
        assert info['n_tiles'] > -(-sp.M // 128) * -(-sp.N // 128)        # more pieces than the uncut tiling has tiles


@pytest.mark.parametrize('entry', ENTRIES)
def test_xcd_dealing(bb, entry):
    _assert_clean(bb, _case('xcd'), entry)


@pytest.mark.parametrize('entry', ENTRIES)
def test_skinny_kernel_and_its_neighbours(bb, entry):
    """The streaming kernel with odd ldc and an odd column offset of C (misaligned pair stores), ragged and odd N, several
    segments, alpha = -2 with beta in {0, 0.5} -- and the problems just outside its conditions, which stay on the MFMA path."""
    info = {}
    _assert_clean(bb, _case('skinny'), entry, info=info)
    if entry == 'plan':
        assert info['n_launches'] == 2
    info = {}
    _assert_clean(bb, _case('skinny_neighbour'), entry, info=info)
    if entry == 'plan':
        assert info['n_launches'] == 1


@pytest.mark.parametrize('entry', ENTRIES)
def test_rounded_data_within_the_derived_bound(bb, entry):
    """Graded standard_normal data against np.longdouble: |err| <= (K + 4) u (|alpha| sum|A||B| + |beta||C0|), per element."""
    for name, case in (('small classes', _case('small_class', 'rc', 'normal')),
                       ('class 0 and strips', _case('class0', bb.ctx.n_cu, 'cr', 1.0, 'normal'))):
        rep = _assert_clean(bb, case, entry)
        assert rep.max_ratio <= 1.0
        by_tag = rep.ratio_by_tag(case)
        groups = gc.SMALL_GROUPS if name == 'small classes' else {'128x128 and strips': gc.CLASS0_SHAPES}
        for group, shapes in groups.items():
            print(f'gemm guard ratio [{entry}] {group}: {max(by_tag[f"{M}x{N}"] for M, N in shapes):.4f}')


_device_lost = []       # settings whose child died, hung or reported a device fault: nothing more is started after one


@pytest.mark.parametrize('setting', ['CYB_GEMM_RAGGED=0', 'CYB_GEMM_SKINNY=0', 'CYB_GEMM_XCD=0', 'CYB_GEMM_XCD=1', 'CYB_GEMM_TAILSPLIT=0',
                                     'CYB_GEMM_TAILSPLIT=2', 'CYB_GEMM_SPLITN=1'])
def test_planner_switches(setting):
    """The class-0, tail-split and streaming groups under every planner switch.  The switches are read once per process,
    hence one child per setting, one after the other; after a child that dies of a signal, hangs or reports a device
    fault no further child is started."""
    if _device_lost:
        pytest.fail(f'not started: the child of {_device_lost[0]} lost the device', pytrace=False)
    env = dict(os.environ)
    env.update([setting.split('=')])
    worker = os.path.join(os.path.dirname(__file__), 'gemm_guard_worker.py')
    try:
        r = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _device_lost.append(setting)
        pytest.fail(f'{setting}: the child hung', pytrace=False)
    text = r.stdout[-1000:] + r.stderr[-4000:]
    if r.returncode < 0 or r.returncode in (134, 139) or any(m in r.stderr for m in (
            'illegal memory access', 'HSA_STATUS_ERROR', 'Memory access fault', 'hipErrorLaunchFailure', 'unspecified launch failure')):
        _device_lost.append(setting)
        pytest.fail(f'{setting}: the child lost the device (status {r.returncode})\n' + text, pytrace=False)
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), text
