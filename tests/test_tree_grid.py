"""``cyten_amd.fusion_tree.from_grid`` / ``from_tree_pairs`` / ``eye`` on the numpy stand-in: the loops, tables and records
without a device.  The cases and their tolerances are in tests/tree_grid_cases.py; tests/test_gpu_tree_grid.py runs the same
ones through HipBlockBackend.  Every case runs with the looped ``tree_place_many`` (one call, nothing zero-filled) and on the
backend without it (zeros_many + get_item / set_item per window)."""
import numpy as np
import pytest

import tree_grid_cases as cases
import tree_grid_ref as ref
from cyten_amd import fusion_tree as ft


@pytest.fixture(params=['place', 'loop'])
def nb(request):
    return cases.NumpyGridBackend() if request.param == 'place' else cases.NumpyLoopBackend()


def _one_call(nb):
    """ONE tree_place_many call where the backend has it"""
    if isinstance(nb, cases.NumpyGridBackend):
        assert len(nb.place_calls) == 1
        return nb.place_calls[0]
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# (a) abelian trees against the dense tensor

@pytest.mark.parametrize('kind', cases.KINDS)
@pytest.mark.parametrize('config', cases.ABELIAN_CONFIGS, ids=lambda c: 'x'.join(map(str, c)))
def test_grid_of_abelian_trees_is_the_concatenated_dense_tensor(nb, rng, config, kind):
    _, windows = cases.check_abelian(nb, rng, config, kind)
    records = _one_call(nb)
    if records is not None:
        assert len(records) == sum(1 for w in windows if w.h * w.nq * w.wn > 0)
        assert any(not has_src for _, has_src in records)
    if config[1] > 1:
        assert any(w.nq > 1 and w.src is not None for w in windows)                   # strided column runs under a stacked domain leg


# ---------------------------------------------------------------------------------------------------------------------------
# (b) made-up spaces against the restatement of the reference's loop

@pytest.mark.parametrize('kinds', cases.KINDS)
def test_forests_of_several_trees_match_the_restatement(nb, rng, kinds):
    cases.check_table(nb, rng, kinds)
    _one_call(nb)


@pytest.mark.parametrize('kinds', cases.KINDS)
def test_complex_factors_on_real_and_complex_entries(nb, rng, kinds):
    cases.check_table(nb, rng, kinds, cases.COMPLEX_FACTORS)


def test_real_factors_on_real_entries_stay_float64(nb, rng):
    have = cases.check_table(nb, rng, 'real', cases.REAL_FACTORS)
    assert all(b.dtype == np.float64 for b in have.values())


def test_adjacent_zero_cells_are_merged_and_every_element_is_written_once(rng):
    nb = cases.NumpyGridBackend()
    _, dev, n_cod, n_dom, left, right = cases.table_case(nb, rng, 'real')
    with cases.captured_windows() as seen:
        got = ft.from_grid(nb, dev, n_cod, n_dom, left, right, discard=False)
    (windows,) = seen
    cover = [np.zeros(b.shape, dtype=np.int64) for b in got.blocks]
    for w in windows:
        tile = cover[w.n][w.x0:w.x1, w.y0:w.y1].reshape(w.x1 - w.x0, w.nq, -1)
        tile[w.r0:w.r0 + w.h, :, w.c0:w.c0 + w.wn] += 1
    assert all((c == 1).all() for c in cover)                                          # the windows partition the blocks
    assert not any(np.isnan(b).any() for b in got.blocks)                              # (empty_many hands out NaN)
    # the block of coupled sector 1: entry (0, 1) is None and (0, 2) lacks the block -- the zero cells (0, 1), (0, 2) are one window
    zero = [w for w in windows if w.src is None and w.n == 1]
    cells = sum(1 for w in windows if w.n == 1 and w.src is not None)
    tiles = len(n_cod.tree_blocks[1]) * len(n_dom.tree_blocks[1])
    assert len(zero) == tiles and cells == 4 * tiles
    assert all(w.wn == right[y_key][3] - right[y_key][1] for w in zero
               for y_key in [next(tb.uncoupled[-1] for tb in n_dom.tree_blocks[1] if tb.start == w.y0)])


def test_zero_windows_merge_runs_and_equal_runs_of_consecutive_rows():
    Z = [[1, 1, 0], [1, 1, 0], [0, 1, 1], [0, 0, 0], [1, 0, 1]]
    assert ft._zero_windows([[bool(v) for v in row] for row in Z]) == [(0, 2, 0, 2), (2, 3, 1, 3), (4, 5, 0, 1), (4, 5, 2, 3)]
    assert ft._zero_windows([]) == [] and ft._zero_windows([[True]]) == [(0, 1, 0, 1)]


def test_restatement_of_a_one_by_one_grid_is_the_entry(rng):
    cod, dom = cases.table_side('cod', cases.ROW_M[0]), cases.table_side('dom', cases.COL_M[0])
    data = cases._random_blocks(rng, cod, dom, True)
    left, right = {k: [0, cases.ROW_M[0][k]] for k in 'ab'}, {k: [0, cases.COL_M[0][k]] for k in 'ab'}
    got = ref.from_grid_ref([[ft.TreeTensor(data, cod, dom)]], cod, dom, left, right)
    assert sorted(got) == [(0, 0), (1, 1), (2, 2)] and all(np.array_equal(got[(s, s)], data.blocks[s]) for s in range(3))


# ---------------------------------------------------------------------------------------------------------------------------
# (c) SU(2)

@pytest.mark.parametrize('cplx', [False, True])
def test_su2_grid_through_to_dense_block(nb, rng, cplx):
    cases.check_su2_grid(nb, rng, cplx)


@pytest.mark.parametrize('cplx', [False, True])
def test_su2_direct_sum_adds_the_squared_norms(nb, rng, cplx):
    cases.check_su2_direct_sum(nb, rng, cplx)


@pytest.mark.parametrize('cplx', [False, True])
def test_compose_with_eye_is_the_identity(nb, rng, cplx):
    cases.check_eye(nb, rng, cplx)


# ---------------------------------------------------------------------------------------------------------------------------
# (d) from_tree_pairs

@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('config', cases.TREE_PAIR_CONFIGS, ids=lambda c: 'x'.join(map(str, c)))
def test_tree_pairs_give_the_blocks_they_were_cut_from(nb, rng, config, cplx):
    cases.check_tree_pairs(nb, rng, config, cplx)
    records = _one_call(nb)
    if records is not None:
        assert all(has_src and shape[1] == 1 for shape, has_src in records)            # one copy record per tile, nq = 1


def test_tree_pairs_missing_tiles_absent_sectors_and_errors(nb, rng):
    cases.check_tree_pairs_structure(nb, rng)


# ---------------------------------------------------------------------------------------------------------------------------
# (e) structure and error paths

def test_zero_blocks_are_discarded_unless_asked_otherwise(nb, rng):
    cases.check_discard(nb, rng)


def test_every_error_path_of_from_grid(nb, rng):
    cases.check_errors(nb, rng)
    if isinstance(nb, cases.NumpyGridBackend):
        assert not nb.place_calls                                                      # refused before anything was placed
