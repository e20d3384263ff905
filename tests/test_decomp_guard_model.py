"""The guard-band decomposition cases (tests/decomp_guard_cases.py) on the host: the numpy stand-in is clean on every case
in both gap fills, every kind of fault is flagged with the kind of failure expected for it, and the route mirror puts every
block where the case says it goes -- with the constants it copies read back from the sources."""
import functools

import numpy as np
import pytest

import decomp_guard_cases as dg

CASES = dg.all_cases()
NAMES = [(g, n) for g, cases in CASES.items() for n in cases]


@functools.lru_cache(maxsize=None)
def _case(group, name, strided=True):
    return CASES[group][name](strided=strided)


def _run(case, fault=None, nan=False, launches=1):
    mem = dg.HostMemory()
    return dg.run(case, dg.NumpyDecomp(mem, fault), mem, nan, launches)


def _checked(group, name, fault=None, nan=False):
    case, twin = _case(group, name), _case(group, name, False)
    return dg.check(case, _run(case, fault, nan), (twin, _run(twin, fault)), nan)


@pytest.mark.parametrize('group,name', NAMES)
def test_the_stand_in_is_clean(group, name):
    """All four checks and the exact structure facts, LAPACK held to an eighth of the cap; the NaN-gap variant gives the
    same bits as the finite one."""
    case = _case(group, name)
    rep = _checked(group, name)
    assert rep.clean, str(rep)
    worst = max((v for m in rep.measures for v in m.values()), default=0.0)
    assert worst <= dg.dac.CAP_EPS / 8, worst
    got, got_nan = _run(case), _run(case, nan=True)
    assert np.array_equal(got.aout, got_nan.aout) and (got.status, got.info, got.rank) == (got_nan.status, got_nan.info, got_nan.rank)
    assert _checked(group, name, nan=True).clean


def test_geometry_of_every_view():
    """Float64 views start 8-byte but not 16-byte aligned, complex views 16-byte aligned; every leading dimension of a matrix
    is odd and above its extent; at least 64 bytes of its own parent lie before and after every view; the contiguous twin
    has ld == extent and 16-byte aligned views."""
    for group, name in NAMES:
        for strided in (True, False):
            case = _case(group, name, strided)
            for b in case.blocks:
                for key, mat in [('A', b.A)] + list(b.out.items()):
                    if mat is None:
                        continue
                    vector = key in ('S', 'W')
                    assert mat.gbyte % 16 == (8 if mat.es == 8 and strided else 0), (name, key)
                    if strided and not vector:
                        assert mat.ld % 2 == 1 and mat.ld > mat.cols
                    else:
                        assert mat.ld == max(mat.cols, 1)
                    span = ((mat.rows - 1) * mat.ld + mat.cols) * mat.es if mat.rows and mat.cols else 0
                    assert mat.gbyte - mat.parent[0] >= 64 and mat.parent[1] - (mat.gbyte + span) >= 64
            assert case.addressed.sum() == sum(m.rows * m.cols * m.es for b in case.blocks for m in b.out.values() if m is not None)


def _fault_targets(kind):
    """(group, case, block) to try a fault on."""
    if kind == 'scale_in_place':
        return [('svd', 'range scale', 0), ('eigh', 'range scale', 0), ('qr', 'range scale, economic', 0)]
    if kind == 'r_lower_unwritten':
        return [('qr', 'unblocked, economic', 1), ('qr', 'blocked, full', 2), ('complex', 'qr small, full', 0)]
    if kind == 's_pad_64':
        return [('svd', 'tiny', 2), ('eigh', 'jacobi', 1), ('complex', 'svd small', 0)]
    return [('svd', 'tiny', 3), ('svd', 'pipeline + direct', 2), ('svd', 'pipeline + direct', 3), ('eigh', 'small', 2),
            ('qr', 'unblocked, economic', 1), ('qr', 'blocked, economic', 1), ('complex', 'svd large', 2), ('complex', 'qr large, full', 1)]


@pytest.mark.parametrize('kind', dg.FAULT_KINDS)
def test_every_fault_is_flagged(kind):
    """On every target, with the kind of failure expected for it; a read from a gap also shows in the NaN variant (a NaN
    block: info = -1 and CYB_ERR_NOCONV, or a poisoned result)."""
    assert set(dg.FAULT_FLAGGED_AS) == set(dg.FAULT_KINDS)
    for group, name, block in _fault_targets(kind):
        rep = _checked(group, name, {'kind': kind, 'block': block})
        assert dg.FAULT_FLAGGED_AS[kind] in rep.failed(), f'{kind} on {name} block {block}: {rep}'
        if kind in ('gap_read', 'lda_as_n'):
            rep = _checked(group, name, {'kind': kind, 'block': block}, nan=True)
            assert rep.failed() & {'status', 'measure', 'structure'}, f'{kind} on {name} block {block}, NaN gaps: {rep}'


def test_the_route_mirror():
    """Every block of every case goes where the case says; the lists named after a route reach it on both sides of its
    threshold; the constants are those of the sources."""
    got = dg.source_constants()
    for key, val in got.items():
        want = {'CSMALL_MAXN': dg.SMALL_MAXN, 'CSMALL_MAXM': dg.SMALL_MAXM}.get(key, getattr(dg, key, None))
        assert val == want, (key, val, want)
    seen = set()
    for group, name in NAMES:
        case = _case(group, name)
        assert case.routes() == case.expect_routes, (name, case.routes())
        assert _case(group, name, False).routes() == case.expect_routes
        seen |= {(case.kind, r) for r in case.routes()}
    for kind, rts in (('svd', ('tiny', 'pipeline', 'direct', 'empty')), ('svd_ex', ('pipeline', 'direct')), ('eigh', ('small', 'jacobi')),
                      ('eigh_ex', ('jacobi',)), ('qr', ('unblocked', 'blocked')), ('csvd', ('small', 'large')), ('ceigh', ('small', 'large')),
                      ('cqr', ('small', 'large'))):
        assert all((kind, r) in seen for r in rts), (kind, rts)
    assert dg.routes('svd', [(64, 128)]) == ['tiny'] and dg.routes('svd', [(65, 65)]) == ['pipeline']
    assert dg.routes('svd', [(64, 129), (1, 200)]) == ['pipeline', 'direct']
    assert dg.routes('svd', [(3, 3)] * 15 + [(65, 65)]) == ['pipeline'] * 16
    assert dg.routes('svd', [(3, 3)] * 16 + [(65, 65)]) == ['tiny'] * 16 + ['pipeline']
    assert dg.routes('eigh', [(64, 64)]) == ['small'] and dg.routes('eigh', [(3, 3), (65, 65)]) == ['jacobi'] * 2
    assert dg.routes('qr', [(95, 200), (96, 96)]) == ['unblocked', 'blocked']
    assert dg.routes('csvd', [(64, 64), (48, 96), (40, 128), (64, 128), (3, 129)]) == ['small'] * 3 + ['large'] * 2
    assert dg.routes('cqr', [(96, 96), (97, 96), (10, 129)]) == ['small', 'large', 'small']
    assert dg.routes('cqr', [(10, 129), (97, 5)], full=1) == ['small', 'large']


def test_a_second_launch_gives_the_same_bytes():
    for group, name in (('svd', 'tiny'), ('qr', 'unblocked, full')):
        case = _case(group, name)
        assert np.array_equal(_run(case).aout, _run(case, launches=2).aout)
