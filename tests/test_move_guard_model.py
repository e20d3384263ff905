"""The guard-band cases of the data-movement kernels (tests/move_guard_cases.py) against the numpy stand-in: the stand-in
passes every case the device test runs, every way these kernels can be wrong is flagged in the Report field it belongs
to, and two of them pass the comparisons the wrapper-level tests make today.  This is the proof that
tests/test_gpu_move_guard.py can fail; no kernel is altered for it."""
import numpy as np
import pytest

import move_guard_cases as mc

GROUPS = {f'{g}: {name}': build for g, cases in mc.all_cases().items() for name, build in cases.items()}


def _run(case, fault=None, launches=1):
    mem = mc.HostMemory()
    return mc.run(case, mc.NumpyMove(mem, fault), mem, launches)


def _rec(case, tag):
    return next(i for i, r in enumerate(case.recs) if r['tag'] == tag)


@pytest.mark.parametrize('name', list(GROUPS))
def test_stand_in_passes_every_case(name):
    case = GROUPS[name]()
    rep = mc.check(case, _run(case))
    assert rep.clean, str(rep)


def test_arenas_are_guarded_unique_and_placed_as_asked():
    case = mc.copy_row_case(8)
    out = case.aout0.view(np.float64)
    assert np.isfinite(out).all() and np.unique(out).size == out.size           # distinct finite doubles everywhere
    src = case.ain.view(np.float64)
    assert np.unique(src).size == src.size
    assert not case.addressed.all() and case.addressed.any()
    for r, (start, end, origin) in zip(case.recs, case.parents):
        lo = min(0, (r['shape'][0] - 1) * r['ds'][0])
        assert origin + 8 * lo - start >= 64 and not case.addressed[start:origin + 8 * lo].any()      # a guard band before
        assert not case.addressed[end - 64:end].any()                                                 # and one after
    starts = {(r['dst'][1] % 16, r['src'][1] % 16) for r in case.recs if r['tag'] in ('16', '17', '2048')}
    assert starts == {(0, 0), (8, 8), (0, 8), (8, 0)}
    gaps = mc.copy_composite_case(4)
    assert not gaps.addressed.all()
    bytes1 = mc.copy_row_case(1)
    assert np.unique(bytes1.aout0).size == 256                                  # a byte stream, not a constant


def test_every_copy_class_is_reached_for_every_element_size():
    """From the classification alone (the mirror of normalize_copy / classify_transpose): a threshold that moves shows
    up as a class no case reaches."""
    cover = mc.copy_coverage()
    for es in (1, 4, 8, 16):
        tiled = 'tiled64' if es == 8 else 'tiled32'
        for cls in ('row', 'shared-row', 'elementwise', tiled, 'composite', 'composite S', 'composite D', 'composite S and D'):
            assert cover.get((es, cls)), f'no case reaches the {cls} class with {es}-byte elements'
        assert (es, 'tiled32' if es == 8 else 'tiled64') not in cover
        print(f'elem_size {es}: ' + '; '.join(f'{cls}: {", ".join(cover[(es, cls)])}' for cls in ('row', 'shared-row', 'elementwise', tiled, 'composite')))


def test_classification_at_its_thresholds():
    cls = lambda *a: mc.classify_copy(*a).name     # noqa: E731
    assert [cls((3, L), (L + 3, 1), (L + 5, 1), 8) for L in (15, 16, 2047, 2048)] == ['elementwise', 'row', 'row', 'shared-row']
    assert cls((3, 40), (43, 1), (41, 1), 16, 1) == 'elementwise' and cls((3, 40), (43, 1), (41, 1), 16, 0) == 'row'
    assert cls((15, 64), (70, 1), (1, 17), 8) == 'elementwise' and cls((64, 15), (17, 1), (1, 70), 8) == 'elementwise'
    assert cls((16, 16), (18, 1), (1, 18), 8) == 'tiled64' and cls((16, 16), (18, 1), (1, 18), 4) == 'tiled32'
    assert cls((4, 5, 6), (30, 6, 1), (30, 6, 1), 1) == 'row' and cls((3, 0, 4), (8, 4, 1), (8, 4, 1), 8) == 'empty'
    # more tiles than one item holds, with a ragged last item (4 tiles of 64 x 64, 16 of 32 x 32 per item)
    t64 = mc.classify_copy((129, 129), (131, 1), (1, 131), 8)
    t32 = mc.classify_copy((129, 129), (131, 1), (1, 131), 16)
    assert (t64.tiles, t32.tiles) == (9, 25)
    both = mc.classify_copy((2, 40, 3, 7), (840, 21, 7, 1), (1, 2, 80, 240), 8)
    assert both.composite and (both.tiled['nD2'], both.tiled['nS2'], both.tiled['nD'], both.tiled['nS']) == (7, 2, 21, 80)


# (fault kind, case builder, tag of the record, Report field)
FAULTS = [
    ('past_row', lambda: mc.copy_row_case(8), '17', 'sentinel'),
    ('past_row', lambda: mc.copy_row_case(1), '256', 'sentinel'),
    ('past_row', lambda: mc.mask_case(False), 'inner 17 outer 3 first and last', 'sentinel'),
    ('past_row', lambda: mc.mask_case(True), 'inner 16 outer 1 one', None),        # inside `out`: the next row is not zero
    ('odd_tail', lambda: mc.copy_row_case(8), '257', 'interior'),
    ('odd_tail', lambda: mc.mask_case(False), 'inner 17 outer 1 all', 'interior'),
    ('j1_eq_j0', lambda: mc.scale_case(False), '(3, 5, 1) x0 out0', 'interior'),
    ('j1_eq_j0', lambda: mc.scale_case(True), '(2, 3, 7) x0 out0', 'interior'),
    ('expand_sign', mc.cexpand_case, '5x3 transposed', 'interior'),
    ('expand_sign', mc.cexpand_real_case, '33x29 sub-view real', 'interior'),
    ('no_conj', lambda: mc.copy_transpose_case(16, True, 1), '33x17', 'interior'),
    ('no_conj', lambda: mc.copy_elementwise_case(16), 'conj long rows', 'interior'),
    ('composite_div', lambda: mc.copy_composite_case(8), '(2, 5, 37, 41, 2) (3, 4, 0, 2, 1)', 'interior'),
    ('composite_div', lambda: mc.copy_composite_case(1), 'composite D under an outer axis', 'interior'),
    ('scatter_no_zero', lambda: mc.mask_case(True), 'inner 1 outer 3 one', 'interior'),
    ('src_at_dst_strides', lambda: mc.copy_row_case(8), '16', 'interior'),
    ('src_at_dst_strides', lambda: mc.lincomb_case(False), '(3, 4, 5, 6) terms 1 acc 0', 'interior'),
    ('src_at_dst_strides', lambda: mc.lincomb_case(True), '(3, 4, 5, 6) terms 3 acc 1', 'interior'),
]


@pytest.mark.parametrize('kind,build,tag,category', FAULTS, ids=[f'{f[0]}-{i}' for i, f in enumerate(FAULTS)])
def test_every_injected_fault_is_reported_in_its_category(kind, build, tag, category):
    case = build()
    rec = _rec(case, tag)
    rep = mc.check(case, _run(case, {'kind': kind, 'rec': rec}))
    hit = {k: bool(getattr(rep, k)) for k in ('interior', 'sentinel', 'source')}
    if category is None:            # one element past a scattered row lands inside `out`, where a zero belongs
        category = 'interior'
    assert hit == {k: k == category for k in hit}, str(rep)
    assert getattr(rep, category)[0][0] == rec
    if kind == 'past_row' and category == 'sentinel':
        r = case.recs[rec]
        end = r['shape'][-1] if case.op == 'copy' else r['outer'] * r['n_keep'] * r['inner']
        # the one element after the first row of a strided destination / after the last row of a gathered block
        assert rep.sentinel[0][1] == end and rep.n_bad['sentinel'] <= case.elem_size


def test_every_fault_kind_has_a_case():
    assert {f[0] for f in FAULTS} == set(mc.FAULT_KINDS)


def test_what_the_wrapper_level_comparisons_let_through():
    """The wrapper-level tests compare the view they asked for, and the complex expansion only behind a GEMM at
    1e-10 * max|ref|: a write past a row and the sign of the -0.0 / +0.0 imaginary parts of a promoted real operand pass
    those; everything else fails them too."""
    passed = {}
    for kind, build, tag, _ in FAULTS:
        case = build()
        got = _run(case, {'kind': kind, 'rec': _rec(case, tag)})
        assert not mc.check(case, got).clean
        ok = mc.cexpand_normwise_ok(case, got) if case.op == 'cexpand' else mc.view_only_ok(case, got)
        passed.setdefault(kind, []).append(ok)
    assert passed['past_row'] == [True, True, True, False]
    assert passed['expand_sign'] == [False, True]
    for kind in ('odd_tail', 'j1_eq_j0', 'no_conj', 'composite_div', 'scatter_no_zero', 'src_at_dst_strides'):
        assert not any(passed[kind]), kind


def test_a_second_launch_changes_nothing_but_an_in_place_scale():
    for build in (lambda: mc.copy_composite_case(8), lambda: mc.mask_case(True), mc.cexpand_case, lambda: mc.lincomb_case(True)):
        case = build()
        if case.op.startswith('lincomb'):
            continue                                   # accumulate = 1 records add twice: not idempotent by design
        assert mc.check(case, _run(case, launches=2)).clean
    case = mc.scale_case(True)
    got = _run(case, launches=2)
    assert mc.check(case, got).interior and not mc.check(case, got).sentinel
    assert mc.check(case, got, mc.scale_twice_expect(case)).clean


def test_misaligned_expand_descriptors_move_one_pointer():
    case = mc.cexpand_case()
    good, n = case.descriptors(1 << 20, 1 << 24)
    for which in ('src', 'dst'):
        bad, _ = mc.cexpand_misaligned(case, which)(1 << 20, 1 << 24)
        diff = [(getattr(a, 'src') - getattr(b, 'src'), getattr(a, 'dst') - getattr(b, 'dst')) for a, b in zip(bad, good)][:n]
        assert sorted(set(diff)) == sorted({(0, 0), (8, 0) if which == 'src' else (0, 8)}) and sum(d != (0, 0) for d in diff) == 1
