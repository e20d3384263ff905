"""The guard-band GEMM cases (tests/gemm_guard_cases.py) against a numpy stand-in for the kernel: the stand-in passes
every case the device tests run, and each way a tile kernel can be subtly wrong is flagged by the checker in its own
category.  This is the proof that tests/test_gpu_gemm_guard.py can fail."""
import numpy as np
import pytest

import gemm_guard_cases as gc

N_CU = 8        # stand-in for the device's CU count (the sizes that depend on it stay small here)


def _run(specs, fault=None, launches=1, seed=3):
    case = gc.build_case(specs, seed)
    mem = gc.HostMemory()
    got = gc.run(case, gc.NumpyGemm(mem, fault), mem, launches)
    return case, got


def test_buffers_are_misaligned_padded_and_poisoned():
    case = gc.build_case([gc.spec(5, 7, (4, 0, 3), 'rc', 1.0, 0.0), gc.spec(6, 4, 3, 'cr', 1.0, 0.5), gc.spec(3, 3, ())], 1)
    for s in case.segs:
        if s.K == 0:
            assert s.a_off < 0 and s.b_off < 0
            continue
        assert s.a_off % 2 == 1 and s.b_off % 2 == 1                        # 8-byte, not 16-byte aligned
        assert sorted((s.a_rs, s.a_cs))[0] == 1 and sorted((s.b_rs, s.b_cs))[0] == 1
        assert max(s.a_rs, s.a_cs) % 2 == 1 and max(s.b_rs, s.b_cs) % 2 == 1
    assert [(s.a_cs == 1, s.b_cs == 1) for s in case.segs if s.K] == [(True, False), (True, True), (False, True)]
    n_view = sum(s.K * (p.spec.M + p.spec.N) for p in case.probs for s in case.segs[p.seg_begin:p.seg_end])
    assert np.isfinite(case.ain).sum() == n_view                            # everything outside the views is NaN
    for p in case.probs:
        M, N = p.spec.M, p.spec.N
        assert p.c_off % 2 == 1 and p.ldc % 2 == 1 and p.ldc > N
        inner = gc._view(case.cout0, p.c_off, (M, N), (p.ldc, 1))
        assert np.isnan(inner).all() if p.spec.beta == 0 else np.isfinite(inner).all()
        assert not gc._view(case.guard, p.c_off, (M, N), (p.ldc, 1)).any()
    assert case.guard.sum() == case.cout0.size - sum(p.spec.M * p.spec.N for p in case.probs)
    assert (case.cout0[case.guard] == gc.SENTINEL).all()
    with pytest.raises(ValueError):
        gc.build_case([gc.spec(4, 4, (300, 300))])                          # total K beyond the exactness argument


def test_exact_data_has_one_result_in_any_summation_order():
    """The premise of the bitwise comparison: forward, backward and pairwise sums over k, and a split over the segments
    in either order, give the reference bit for bit."""
    case = gc.build_case([gc.spec(33, 47, (33, 2, 48), 'rc', -2.0, 0.5), gc.spec(19, 300, 69, 'cc', 0.5, 1.0)], 5)
    for p in case.probs:
        M, N = p.spec.M, p.spec.N
        terms = []
        for s in case.segs[p.seg_begin:p.seg_end]:
            A = gc._view(case.ain, s.a_off, (M, s.K), (s.a_rs, s.a_cs))
            B = gc._view(case.ain, s.b_off, (s.K, N), (s.b_rs, s.b_cs))
            terms += [np.outer(A[:, k], B[k, :]) for k in range(s.K)]
        C0 = gc._view(case.cout0, p.c_off, (M, N), (p.ldc, 1))
        fwd = sum(terms[1:], terms[0])
        bwd = sum(terms[-2::-1], terms[-1])
        pair = list(terms)
        while len(pair) > 1:
            pair = [pair[i] + pair[i + 1] if i + 1 < len(pair) else pair[i] for i in range(0, len(pair), 2)]
        for acc in (fwd, bwd, pair[0]):
            assert np.array_equal(p.spec.alpha * acc + p.spec.beta * C0, p.ref)


GROUPS = {
    'small rr': lambda: gc.small_class_specs('rr'),
    'small rc': lambda: gc.small_class_specs('rc'),
    'small cr': lambda: gc.small_class_specs('cr'),
    'small cc': lambda: gc.small_class_specs('cc'),
    'class0 rr beta0': lambda: gc.class0_specs(N_CU, 'rr', 0.0),
    'class0 cr beta1': lambda: gc.class0_specs(N_CU, 'cr', 1.0),
    'degenerate': gc.degenerate_specs,
    'many tiles': lambda: gc.many_tiles_specs(N_CU),
    'tail split': lambda: gc.tail_split_specs(N_CU),
    'xcd': gc.xcd_specs,
    'skinny': gc.skinny_specs,
    'skinny neighbours': gc.skinny_neighbour_specs,
}


@pytest.mark.parametrize('group', list(GROUPS))
def test_stand_in_passes_every_exact_group(group):
    case, got = _run(GROUPS[group]())
    rep = gc.check(case, got)
    assert rep.clean, str(rep)
    assert rep.max_ratio == 0.0


def test_plan_run_twice_accumulates_twice():
    specs = gc.many_tiles_specs(N_CU)
    case, got = _run(specs, launches=2)
    once = gc.check(case, got)
    assert once.interior and not once.nan and not once.sentinel            # C0 + A B is NOT what two runs leave
    refs = [2 * p.ref - gc._view(case.cout0, p.c_off, (p.spec.M, p.spec.N), (p.ldc, 1)) for p in case.probs]   # C0 + 2 A B
    assert gc.check(case, got, refs).clean


def test_stand_in_meets_the_derived_bound_on_rounded_data():
    specs = gc.small_class_specs('rc', 'normal')[::7] + gc.class0_specs(N_CU, 'cr', 1.0, 'normal')[::5]
    case, got = _run(specs)
    rep = gc.check(case, got)
    assert rep.clean, str(rep)
    assert 0.0 < rep.max_ratio <= 1.0
    # an error of a few ulps OF THE ELEMENT is inside the bound only while it stays below (K + 4) u sum|a||b|
    p = case.probs[1]
    bad = got.copy()
    gc._view(bad, p.c_off, (p.spec.M, p.spec.N), (p.ldc, 1))[0, 0] += float(2 * p.bound[0, 0])
    rep = gc.check(case, bad)
    assert rep.interior and rep.interior[0][:3] == (1, 0, 0) and rep.max_ratio > 1.0


def test_longdouble_guard_refuses_a_narrow_type(monkeypatch):
    class Narrow:
        eps = 2.0 ** -52
    monkeypatch.setattr(np, 'finfo', lambda t: Narrow)
    with pytest.raises(RuntimeError, match='longdouble'):
        gc.require_longdouble()


# one problem per tile regime, graded so that row `small` is the one a normwise tolerance cannot see
FAULT_SPECS = [gc.spec(129, 127, 17, 'rc', 1.0, 0.0), gc.spec(263, 307, 90, 'cr', 0.5, -2.0), gc.spec(33, 47, (33, 2, 45), 'cc', -2.0, 1.0)]


def _smallest_row(case, pi):
    p = case.probs[pi]
    return int(np.argmin(np.abs(p.ref).max(axis=1) + (np.abs(p.ref).max(axis=1) == 0) * 1e300))


FAULTS = [('drop_last_k_of_row', 'interior'), ('drop_k_tail', 'interior'), ('skip_tile', None), ('tile_twice', 'interior'),
          ('store_col_N', 'sentinel'), ('store_row_M', 'sentinel'), ('read_row_M', 'nan'), ('read_col_K', 'nan'), ('read_c_beta0', 'nan')]
# (a tile applied twice needs beta != 0 to show, and C is read legitimately then: those pairs are not generated)
FAULT_PARAMS = [(kind, cat, pi) for kind, cat in FAULTS for pi, sp in enumerate(FAULT_SPECS)
                if not (kind == 'tile_twice' and sp.beta == 0) and not (kind == 'read_c_beta0' and sp.beta != 0)]


@pytest.mark.parametrize('kind,category,pi', FAULT_PARAMS)
def test_every_injected_fault_is_reported_in_its_category(kind, category, pi):
    clean = gc.build_case(FAULT_SPECS, 3)
    sp = FAULT_SPECS[pi]
    if kind == 'skip_tile':
        category = 'nan' if sp.beta == 0 else 'interior'          # a skipped tile leaves what was there: NaN, or C0
    row = _smallest_row(clean, pi)
    fault = {'kind': kind, 'prob': pi, 'row': row, 'col': sp.N // 2, 'rows': (16, 32), 'cols': (16, 32)}
    case, got = _run(FAULT_SPECS, fault)
    rep = gc.check(case, got)
    hit = {k: bool(getattr(rep, k)) for k in ('interior', 'nan', 'sentinel')}
    assert hit == {k: k == category for k in hit}, str(rep)
    first = getattr(rep, category)[0]
    assert first[0] == pi
    if kind in ('drop_last_k_of_row', 'read_col_K'):
        assert first[1] == row
    if kind == 'read_row_M':
        assert first[1] == sp.M - 1
    if kind in ('skip_tile', 'tile_twice'):
        assert first[1:3] == (16, 16) and rep.n_bad[category] <= 256
    if kind == 'store_col_N':
        assert first[1] == row * case.probs[pi].ldc + sp.N
    if kind == 'store_row_M':
        assert first[1] == sp.M * case.probs[pi].ldc + sp.N // 2


@pytest.mark.parametrize('pi', [0, 1])
def test_the_normwise_tolerance_misses_what_the_exact_check_finds(pi):
    """The reason for this suite: one lost term of a small-magnitude row is far
    below `1e-10 * max|ref|` (tests/test_gpu_gemm.py) and is a plain mismatch for the bitwise comparison."""
    clean = gc.build_case(FAULT_SPECS, 3)
    row = _smallest_row(clean, pi)
    case, got = _run(FAULT_SPECS, {'kind': 'drop_last_k_of_row', 'prob': pi, 'row': row})
    assert gc.normwise_ok(case, got)
    rep = gc.check(case, got)
    assert rep.interior and rep.interior[0][:2] == (pi, row)
    p = case.probs[pi]
    err = abs(rep.interior[0][3] - rep.interior[0][4])
    assert err <= 1e-14 * np.abs(p.ref).max()                    # orders of magnitude under the old tolerance
