"""The batched decompositions at the C ABI on guard-band cases (tests/decomp_guard_cases.py): every A, U, S, Vh, W, V, Q
and R a strided, oddly aligned view into a larger arena, in ONE call per case, with finite values and with NaN in every gap
of the inputs.  Every byte around the results and every source is compared with what was uploaded, the results themselves
bit for bit with the same list decomposed from contiguous copies in the same process, and held to the 1e-13 of
tests/decomp_accuracy_cases.py; the structural facts are exact.  tests/test_decomp_guard_model.py shows on the host that
each kind of fault is flagged and which route every block takes.  Every case prints its largest measures in eps = 2^-52."""
import functools

import pytest

import decomp_guard_cases as dg
from decomp_guard_worker import launcher, run_case, untouched, uploaded

pytestmark = pytest.mark.gpu

CASES = dg.all_cases()


@functools.lru_cache(maxsize=None)
def _case(group, name, strided=True):
    """Cases are immutable (a run uploads copies of the arenas)."""
    return CASES[group][name](strided=strided)


def _assert_clean(bb, group, name, launches=1):
    case, twin = _case(group, name), _case(group, name, False)
    twin_got = run_case(bb, twin)
    for nan in (False, True):
        got = run_case(bb, case, nan, launches)
        rep = dg.check(case, got, (twin, twin_got), nan)
        worst = {}
        for m in rep.measures:
            for key, val in m.items():
                key = 'orth' if key.startswith('orth') else key
                worst[key] = max(worst.get(key, 0.0), val)
        print(f'[guard] {group:8s} {name:40s} {"NaN gaps" if nan else "finite  "} ' + '  '.join(f'{k} {v:8.2f}' for k, v in sorted(worst.items())))
        assert rep.clean, f'{name} ({"NaN" if nan else "finite"} gaps): {rep}'
    return got


@pytest.mark.parametrize('name', list(CASES['svd']))
def test_real_svd(bb, name):
    """The in-LDS route, pipeline and direct route in one call (plain, and with CYB_SVD_SKIP_NULL_VECTORS and rank), the
    in-LDS route beside the pipeline, embedded complex blocks, a range-scaled block on either route."""
    got = _assert_clean(bb, 'svd', name)
    case = _case('svd', name)
    if case.want_rank:          # where the route shows at the ABI: the pipeline reports the numerical rank, the others k
        for b, route, rank in zip(case.blocks, case.routes(), got.rank):
            assert rank == (10 if b.tag == 'rank 10' else min(b.m, b.n)), (b.m, b.n, route, rank)
            assert route == 'pipeline' or b.tag != 'rank 10'


@pytest.mark.parametrize('name', list(CASES['eigh']))
def test_real_eigh(bb, name):
    """The in-LDS route and run_jacobi, with V and with V = NULL, embedded complex blocks, a range-scaled block."""
    _assert_clean(bb, 'eigh', name)


@pytest.mark.parametrize('name', list(CASES['qr']))
def test_real_qr(bb, name):
    """The one-workgroup Householder kernel and the blocked route, economic and full, and the in-place rescale of R over ldr."""
    _assert_clean(bb, 'qr', name)


@pytest.mark.parametrize('name', list(CASES['complex']))
def test_complex_entries(bb, name):
    """cyb_{svd,eigh,qr}_batched_c128 on either side of each small-route limit."""
    _assert_clean(bb, 'complex', name)


@pytest.mark.parametrize('group,name', [('svd', 'tiny + pipeline'), ('eigh', 'jacobi'), ('qr', 'blocked, full'), ('complex', 'svd large')])
def test_a_second_launch_gives_the_same_bytes(bb, group, name):
    _assert_clean(bb, group, name, launches=2)


REFUSALS = [   # (entry, shapes of the list, flags or `full`, the block, its output leading dimensions)
    ('svd', [(65, 65)], 0, 0, ('ldu', 'ldvh')),                        # pipeline
    ('svd', [(1, 200)], 0, 0, ('ldu', 'ldvh')),                        # direct
    ('svd', [(5, 3)], 0, 0, ('ldu', 'ldvh')),                          # in-LDS
    ('svd', [(3, 3)] * 16 + [(65, 65)], 0, 16, ('ldu', 'ldvh')),       # the pipeline's block behind sixteen in-LDS blocks
    ('svd_ex', [(66, 66)], dg.EMBEDDED, 0, ('ldu', 'ldvh')),
    ('eigh', [(65, 65)], 0, 0, ('ldv',)),                              # run_jacobi
    ('eigh', [(9, 9)], 0, 0, ('ldv',)),                                # in-LDS
    ('eigh_ex', [(66, 66)], dg.EMBEDDED, 0, ('ldv',)),
    ('qr', [(6, 4)], 0, 0, ('ldq', 'ldr')), ('qr', [(96, 96)], 1, 0, ('ldq', 'ldr')),
    ('csvd', [(5, 3)], 0, 0, ('ldu', 'ldvh')), ('csvd', [(65, 65)], 0, 0, ('ldu', 'ldvh')),
    ('ceigh', [(9, 9)], 0, 0, ('ldv',)), ('ceigh', [(65, 65)], 0, 0, ('ldv',)),
    ('cqr', [(4, 6)], 0, 0, ('ldq', 'ldr')), ('cqr', [(97, 97)], 1, 0, ('ldq', 'ldr')),
]


def _refusal_case(kind, shapes, opt):
    if kind in ('qr', 'cqr'):
        return dg._qr_case('refusal', shapes, [], kind, full=opt)
    if kind in ('eigh', 'eigh_ex', 'ceigh'):
        return dg._eigh_case('refusal', [n for _, n in shapes], [], kind, opt)
    return dg._svd_case('refusal', shapes, [], kind, opt)


@pytest.mark.parametrize('kind,shapes,opt,block,fields', REFUSALS, ids=[f'{r[0]} {r[1][-1][0]}x{r[1][-1][1]} of {len(r[1])}' for r in REFUSALS])
def test_short_output_leading_dimensions_are_refused(bb, kind, shapes, opt, block, fields):
    """ldu = k - 1, ldvh = n - 1, ldv = n - 1, ldq = kq - 1 and ldr = n - 1 are each CYB_ERR_INVALID on every route of every
    entry, and both arenas are byte for byte what was uploaded after every refused call."""
    case = _refusal_case(kind, shapes, opt)
    assert case.routes()[block] != 'empty'
    mem, bases = uploaded(bb, case)
    launch = launcher(bb)
    b = case.blocks[block]
    bound = {'ldu': min(b.m, b.n), 'ldvh': b.n, 'ldv': b.n, 'ldq': b.m if b.full else min(b.m, b.n), 'ldr': b.n}
    for f in fields:
        descs = case.descriptors(*bases)
        setattr(descs[block], f, bound[f] - 1)
        st, _, _ = launch(kind, descs, len(case.blocks), case.flags, case.family != 'qr', False)
        assert st == dg.CYB_ERR_INVALID, (kind, shapes[block], f, st)
        assert b'leading dimension' in bb.lib.cyb_last_error(), bb.lib.cyb_last_error()
        assert untouched(mem, bases, case), (kind, shapes[block], f)
    descs = case.descriptors(*bases)                     # the same descriptors as they were: accepted
    st, _, _ = launch(kind, descs, len(case.blocks), case.flags, case.family != 'qr', False)
    assert st == dg.CYB_OK


@pytest.mark.parametrize('sizes', [(65, 3), (9, 3)], ids=['run_jacobi', 'in-LDS'])
def test_eigenvalues_alone_ignore_ldv(bb, sizes):
    """V = NULL with any ldv is accepted, and gives the eigenvalues of the call with V bit for bit."""
    case = dg._eigh_case('no V', sizes, [], no_v=True)
    want = run_case(bb, case)
    assert want.status == dg.CYB_OK
    for ldv in (0, -3, 1 << 40):
        mem, bases = uploaded(bb, case)
        descs = case.descriptors(*bases)
        for d in descs:
            d.ldv = ldv
        st, _, _ = launcher(bb)('eigh', descs, len(case.blocks), 0, True, False)
        assert st == dg.CYB_OK, ldv
        got = mem.download(bases[1], case.aout0.size // 8).view('uint8')
        assert (got == want.aout).all(), ldv
