"""Inputs of the direct-sum tests shared by tests/test_direct_sum.py (numpy stand-in) and tests/test_gpu_direct_sum.py
(HipBlockBackend: the same inputs, the same criteria).

A component ("part") is one of
  'ab2'   a U(1) two-leg tensor X on [a, b*] (bond dimension 33 each; blocks 1 x 5, 9 x 1 and 20 x 7) under X -> A X B, two
          ``ab.tdot`` with charge-conserving Hermitian A and B;
  'ab1'   a U(1) one-leg tensor (its only charge-allowed block: 23 elements) under ``sparse.TensorLinearOperator``;
  'tree'  the fusion-tree spaces and the chain operator of tests/tree_krylov_cases.py.
Every part has its dense form in coordinates y in which the inner product is the plain one -- for a tree part the scaled
coordinates of tests/tree_krylov_ref.py (the weighted metric), for an abelian part the charge-allowed blocks one after the
other.  A :class:`SumCase` puts parts together: the operator H1 (+) H2 (+) ..., its block-diagonal dense matrix and the
vectors.  Every part's operator is Hermitian with ONE eigenvalue `-special^2` (or `special` for 'ab1') set well below the
rest of its spectrum, so that the ground state of a sum is non-degenerate when the parts have different ones."""
import numpy as np
import scipy.linalg as sla

import tree_krylov_cases as tcases
import tree_krylov_ref as ref
from cyten_amd import abelian as ab
from cyten_amd import direct_sum as ds
from cyten_amd import sparse


class NumpyDirectSumBackend(tcases.NumpyKrylovBackend):
    """the stand-in of the tree solvers + the conjugating inner product of abelian block lists"""

    def inner_many(self, xs, ys):
        s = sum(np.vdot(x, y) for x, y in zip(xs, ys))
        return complex(s) if np.iscomplexobj(s) else float(s)


U1 = ab.Symmetry([0])
LEG_A = ab.Leg(U1, [[-1], [0], [1], [2]], [3, 1, 9, 20], +1)
LEG_B = ab.Leg(U1, [[0], [1], [2], [3]], [5, 1, 7, 20], +1)
LEG_C = ab.Leg(U1, [[0], [1]], [23, 5], +1)


def _rand(rng, shape, cplx):
    return rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)


def _diag_operator(bb, rng, leg, cplx, special_at=None, special=None):
    """(two-leg tensor on [leg, leg*] with one Hermitian block per sector, the blocks)"""
    mats = [tcases._hermitian(rng, int(m), cplx, special if k == special_at else None) for k, m in enumerate(leg.mults)]
    inds = [(k, k) for k in range(leg.nsec)]
    return ab.AbelianTensor.from_numpy_blocks(bb, U1, [leg, leg.dual()], mats, inds, 1), mats


def ab_blocks(bb, t, inds):
    """the blocks of `t` on the rows `inds` as numpy arrays, zeros where it has none"""
    have = {tuple(r): np.asarray(bb.to_numpy(b)) for r, b in zip(t.block_inds.tolist(), t.blocks)}
    assert set(have) <= {tuple(r) for r in inds.tolist()}
    return [have.get(tuple(r), np.zeros(t.block_shape(r))) for r in inds.tolist()]


class TwoSided:
    """X -> A X B on two-leg abelian tensors: two contractions on the grouped GEMM"""

    def __init__(self, bb, A, B, is_complex):
        self.bb, self.A, self.B, self.is_complex = bb, A, B, bool(is_complex)

    def matvec(self, x):
        y = ab.tdot(self.bb, ab.tdot(self.bb, self.A, x, [1], [0]), self.B, [1], [0])
        y.num_codomain = x.num_codomain
        return y

    def adjoint(self):
        return TwoSided(self.bb, ab.dagger(self.bb, self.A), ab.dagger(self.bb, self.B), self.is_complex)


class DenseOp:
    """a dense matrix on the coordinates of an abelian part (a host round trip): its result holds EVERY charge-allowed block,
    whatever the input held -- the operator that creates blocks outside the support of a start vector"""

    def __init__(self, part, M):
        self.part, self.M, self.bb, self.is_complex = part, M, part.bb, bool(np.iscomplexobj(M))

    def matvec(self, x):
        return self.part.tensor(self.M @ self.part.y(x))


class AbelianPart:
    def __init__(self, bb, rng, legs, cplx_vec):
        self.bb, self.legs = bb, legs
        self.inds = ab.AbelianTensor.allowed_block_inds(U1, legs)
        self.shapes = [tuple(int(l.mults[i]) for l, i in zip(legs, r)) for r in self.inds]
        self.x0 = [_rand(rng, sh, cplx_vec) for sh in self.shapes]
        self.psi0 = self.tensor_of(self.x0)
        self.y0 = np.concatenate([b.ravel() for b in self.x0])

    def tensor_of(self, blocks, keep=None):
        keep = range(len(blocks)) if keep is None else keep
        return ab.AbelianTensor.from_numpy_blocks(self.bb, U1, self.legs, [blocks[k] for k in keep], self.inds[list(keep)], 1)

    def y(self, t):
        return np.concatenate([b.ravel() for b in ab_blocks(self.bb, t, self.inds)])

    def tensor(self, y, keep=None):
        out, off = [], 0
        for sh in self.shapes:
            n = int(np.prod(sh))
            out.append(np.ascontiguousarray(y[off:off + n].reshape(sh)))
            off += n
        return self.tensor_of(out, keep)

    def expm_apply(self, delta, y):
        return sla.expm(delta * self.M) @ y


class Ab2Part(AbelianPart):
    def __init__(self, bb, rng, cplx_op, cplx_vec, special):
        super().__init__(bb, rng, [LEG_A, LEG_B.dual()], cplx_vec)
        assert self.inds.tolist() == [[1, 0], [2, 1], [3, 2]] and self.shapes == [(1, 5), (9, 1), (20, 7)]
        A, am = _diag_operator(bb, rng, LEG_A, cplx_op, 3, special)
        B, bm = _diag_operator(bb, rng, LEG_B, cplx_op, 2, -special)
        self.H = TwoSided(bb, A, B, cplx_op)
        self.M = sla.block_diag(*[np.kron(am[i], bm[j].T) for i, j in self.inds.tolist()])
        self.E0 = -special * special


class Ab1Part(AbelianPart):
    def __init__(self, bb, rng, cplx_op, cplx_vec, special):
        super().__init__(bb, rng, [LEG_C], cplx_vec)
        assert self.inds.tolist() == [[0]] and self.shapes == [(23,)]
        T, tm = _diag_operator(bb, rng, LEG_C, cplx_op, 0, special)
        self.H = sparse.TensorLinearOperator(bb, T, -1)
        self.M = tm[0]
        self.E0 = special


class TreePart:
    def __init__(self, bb, rng, cplx_op, cplx_vec, special):
        self.bb, self.qdims = bb, tcases.QDIMS
        self.cod, self.dom = tcases.spaces()
        last = len(tcases.ROWS) - 1
        self.A = [tcases._hermitian(rng, r, cplx_op, special if k == last else None) for k, r in enumerate(tcases.ROWS)]
        self.B = [tcases._hermitian(rng, c, cplx_op, -special if k == last else None) for k, c in enumerate(tcases.COLS)]
        self.x0 = tcases.vector_blocks(rng, cplx_vec)
        self.H = tcases.chain(bb, self.A, self.B, self.cod, self.dom)
        self.psi0 = tcases.tree_tensor(bb, self.x0, self.cod, self.dom)
        self.M = ref.dense_operator(self.A, self.B)
        self.y0 = ref.scaled(self.x0, self.qdims)
        self.E0 = -special * special

    def y(self, t):
        return ref.scaled(tcases.host_blocks(self.bb, t), self.qdims)

    def tensor(self, y, keep=None):
        blocks = ref.unscaled(y, tcases.SHAPES, self.qdims)
        if keep is not None:
            blocks = [b if k in keep else None for k, b in enumerate(blocks)]
        return tcases.tree_tensor(self.bb, blocks, self.cod, self.dom)

    def expm_apply(self, delta, y):
        return ref.expm_apply(self.A, self.B, delta, y)


KINDS = {'ab2': Ab2Part, 'ab1': Ab1Part, 'tree': TreePart}
# the three sums of the solver tests, with the value that sets each part's lowest eigenvalue
COMBOS = {'abelian+abelian': (('ab2', 2.0), ('ab1', -5.5)),
          'tree+tree': (('tree', 2.5), ('tree', 2.0)),
          'abelian+tree': (('ab2', 2.0), ('tree', 2.5))}


class SumCase:
    """operator, start vector and their dense forms of a direct sum of parts"""

    def __init__(self, bb, parts, seed=0, cplx_op=False, cplx_vec=False):
        """`parts`: a key of COMBOS or a sequence of (kind, special); `cplx_vec`: a bool, or one per part"""
        parts = COMBOS[parts] if isinstance(parts, str) else parts
        cv = [cplx_vec] * len(parts) if isinstance(cplx_vec, bool) else list(cplx_vec)
        rng = np.random.default_rng(4200 + seed)
        self.bb = bb
        self.parts = [KINDS[kind](bb, rng, cplx_op, c, special) for (kind, special), c in zip(parts, cv)]
        self.H = sparse.DirectSumLinearOperator([p.H for p in self.parts], bb)
        self.psi0 = ds.DirectSum([p.psi0 for p in self.parts])
        self.M = sla.block_diag(*[p.M for p in self.parts])
        self.y0 = np.concatenate([p.y0 for p in self.parts])
        self.bounds = np.concatenate([[0], np.cumsum([len(p.y0) for p in self.parts])])

    def y(self, x):
        assert isinstance(x, ds.DirectSum) and len(x) == len(self.parts)
        return np.concatenate([p.y(c) for p, c in zip(self.parts, x.components)])

    def tensor(self, y):
        return ds.DirectSum([p.tensor(y[a:b]) for p, a, b in zip(self.parts, self.bounds[:-1], self.bounds[1:])])

    def expm_apply(self, delta, y):
        return np.concatenate([p.expm_apply(delta, y[a:b]) for p, a, b in zip(self.parts, self.bounds[:-1], self.bounds[1:])])

    def spectrum(self, k=2):
        """(all eigenvalues of M ascending, its k lowest eigenvectors as columns), part by part: M is their direct sum"""
        if not hasattr(self, '_spec'):
            self._spec = [np.linalg.eigh(p.M) for p in self.parts]
        E = np.concatenate([e for e, _ in self._spec])
        where = np.concatenate([np.full(len(e), i) for i, (e, _) in enumerate(self._spec)])
        local = np.concatenate([np.arange(len(e)) for e, _ in self._spec])
        order = np.argsort(E, kind='stable')
        U = np.zeros((len(self.y0), k), dtype=np.result_type(*[u.dtype for _, u in self._spec]))
        for c, n in enumerate(order[:k]):
            i = where[n]
            U[self.bounds[i]:self.bounds[i + 1], c] = self._spec[i][1][:, local[n]]
        return E[order], U

    def zero_like(self):
        return ds.scale(self.bb, 0.0, self.psi0)


def three_four(bb):
    """a direct sum of two one-leg tensors with the entries 3 and 4: its norm is exactly 5"""
    def one(x):
        b = np.zeros(23)
        b[7] = x
        return ab.AbelianTensor.from_numpy_blocks(bb, U1, [LEG_C], [b], [[0]], 1)
    return ds.DirectSum([one(3.0), one(4.0)])


def component_is_zero(bb, t) -> bool:
    """every block the component holds is exactly zero"""
    return all(not np.any(np.asarray(bb.to_numpy(b))) for b in t.blocks)


def check_ground_state(case, opts, flat=None):
    """the criteria of tree_krylov_cases.check_ground_state with the block-diagonal dense matrix as the yardstick; returns
    (solver, E0, psi, N)"""
    from cyten_amd import krylov
    bb = case.bb
    o = dict(opts, reortho=True)
    if flat is not None:
        o['flat'] = flat
    solver = krylov.LanczosGroundState(bb, case.H, case.psi0, o)
    E0, psi, N = solver.run()
    E, U = case.spectrum()
    assert abs(E0 - E[0]) < 1e-9 * abs(E[0])
    assert abs(abs(np.vdot(U[:, 0], case.y(psi))) - 1.0) < 1e-7
    assert abs(ds.norm(bb, psi) - 1.0) < 1e-12
    h = solver._h[:N + 1, :N + 1]
    want = ref.lanczos_h(case.M, case.y0, N)
    assert np.abs(h - want).max() <= 1e-10 * np.abs(want).max()
    return solver, E0, psi, N
