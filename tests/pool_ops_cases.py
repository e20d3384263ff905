"""The vector operations of the Krylov solvers (cyten_amd.krylov_vectors: ``enter / leave / scale / lincomb / combine / inner /
norm / project_out / rotate / orthonormalize`` and the operator wrappers) method by method against numpy: the cases, the
reference and the checks shared by tests/test_pool_ops.py (the tensor classes on a numpy stand-in) and
tests/test_gpu_pool_ops.py (the pools and the tensor classes on the device).  No device code here: a check talks to an ops
object through its public methods, and reads a pool only by downloading it.

COORDINATES.  A vector of a layout is its blocks one after the other, `u` (the blocks as they are stored) or `y = s * u` with
s = sqrt(quantum dimension) of the block (1 for an abelian block): in `y` the weighted inner product is the plain one and the
operator is the dense matrix `case.M` (tests/direct_sum_cases.py).  Everything linear is compared in `u`, every reduction in
`y`.  The reference is plain numpy in ``np.longdouble`` / ``np.clongdouble``; nothing under test takes part in it.

BOUNDS, with eps = 2**-52:
* a linear combination of k terms (an accumulator counts as one): elementwise ``(k + 3) eps sum_k |c_k| |x_k|`` -- one rounding
  per add and at most sqrt(5) half-ulps per complex product; a rotation by a real m x k matrix: ``(m + 2) eps |Y| @ |Q|``;
* a reduction: ``1e-13 |v| |w|``, a norm ``1e-13`` relative -- the project's bound for these kernels (test_gpu_projection_kernels,
  test_gpu_tree_krylov); Gram-Schmidt steps: the bounds of test_general_weights_against_numpy;
* an operator application: ``1e-12 |M| |y|``.
"""
import math

import numpy as np
import pytest

import direct_sum_cases as dc
import tree_krylov_cases as tcases
from cyten_amd import abelian as ab
from cyten_amd import fusion_tree as ft
from cyten_amd import sparse
from cyten_amd.direct_sum import DirectSum
from cyten_amd.krylov_vectors import _NeedComplex, _NotFlat

EPS = 2.0 ** -52
TAU = 1e-13
THREE = (('ab2', 2.0), ('tree', 2.5), ('ab1', -5.5))
LAYOUTS = {'abelian': (('ab2', 2.0),), 'tree': (('tree', 2.5),), 'abelian+abelian': dc.COMBOS['abelian+abelian'],
           'abelian+tree': dc.COMBOS['abelian+tree'], 'three': THREE}
SINGLE = ('abelian', 'tree')
WEIGHTED = ('tree', 'abelian+tree', 'three')


def ld(a):
    """`a` in extended precision"""
    a = np.asarray(a)
    return a.astype(np.clongdouble if np.iscomplexobj(a) else np.longdouble)


def ld_vdot(a, b):
    """sum conj(a) b accumulated in extended precision"""
    return complex(np.sum(np.conj(ld(a)) * ld(b)))


def ld_norm(a):
    return float(np.sqrt(np.sum(np.abs(ld(a)) ** 2)))


def _random(rng, n, cplx):
    return rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)


class OpsCase:
    """One layout: its parts (tests/direct_sum_cases.py), the template vector, the operator and its dense matrix, and the maps
    between vectors and coordinates."""

    def __init__(self, bb, layout, cplx_op=False):
        self.bb, self.layout, self.is_sum = bb, layout, layout not in SINGLE
        self.sum = dc.SumCase(bb, LAYOUTS[layout], 31, cplx_op)
        self.parts, self.M = self.sum.parts, self.sum.M
        self.template = self.sum.psi0 if self.is_sum else self.parts[0].psi0
        self.H = self.sum.H if self.is_sum else self.parts[0].H
        self.shapes, self.part_of, self.local, scale = [], [], [], []
        for i, p in enumerate(self.parts):
            shapes = [tuple(sh) for sh in (tcases.SHAPES if isinstance(p, dc.TreePart) else p.shapes)]
            qd = p.qdims if isinstance(p, dc.TreePart) else [1.0] * len(shapes)
            for k, (sh, d) in enumerate(zip(shapes, qd)):
                self.shapes.append(sh)
                self.part_of.append(i)
                self.local.append(k)
                scale.append(np.full(math.prod(sh), np.sqrt(d)))
        self.sizes = [math.prod(sh) for sh in self.shapes]
        self.bounds = np.concatenate([[0], np.cumsum(self.sizes)])
        self.s = np.concatenate(scale)
        self.n = len(self.s)
        assert self.n == self.M.shape[0]
        # a strict subset of the blocks that leaves every part at least one: all but the second block of a part that has two
        self.subset = [g for g in range(len(self.shapes)) if self.local[g] != 1]
        assert 0 < len(self.subset) < len(self.shapes)

    def wrap(self, comps):
        return DirectSum(comps) if self.is_sum else comps[0]

    def from_u(self, u, keep=None):
        """the vector with the coordinates `u`, holding only the blocks `keep` (the others must be zero in `u`)"""
        keep = range(len(self.shapes)) if keep is None else keep
        comps = []
        for i, p in enumerate(self.parts):
            mine = [g for g in range(len(self.shapes)) if self.part_of[g] == i]
            blocks = [np.ascontiguousarray(u[self.bounds[g]:self.bounds[g + 1]].reshape(self.shapes[g])) for g in mine]
            held = [k for k, g in enumerate(mine) if g in keep]
            if isinstance(p, dc.TreePart):
                comps.append(tcases.tree_tensor(self.bb, [b if k in held else None for k, b in enumerate(blocks)], p.cod, p.dom))
            else:
                comps.append(p.tensor_of(blocks, held))
        return self.wrap(comps)

    def rand(self, rng, cplx, subset=False):
        """(vector, u): random coordinates, on all blocks or on `self.subset` only"""
        u = _random(rng, self.n, cplx)
        if subset:
            mask = np.zeros(self.n, dtype=bool)
            for g in self.subset:
                mask[self.bounds[g]:self.bounds[g + 1]] = True
            u = np.where(mask, u, 0.0)
        return self.from_u(u, self.subset if subset else None), u

    def from_y(self, y):
        """(vector, u) of the scaled coordinates `y`"""
        u = y / self.s
        return self.from_u(u), u

    def u(self, x):
        """the coordinates of a vector (zeros where it holds no block)"""
        comps = x.components if self.is_sum else [x]
        assert len(comps) == len(self.parts)
        out = []
        for p, t in zip(self.parts, comps):
            blocks = tcases.host_blocks(self.bb, t) if isinstance(p, dc.TreePart) else dc.ab_blocks(self.bb, t, p.inds)
            out += [np.asarray(b).ravel() for b in blocks]
        return np.concatenate(out)

    def other_shape(self, rng):
        """a vector of this kind whose first part has the block rows of the layout and another block shape"""
        p = self.parts[0]
        if isinstance(p, dc.TreePart):
            rows = [r + 1 for r in tcases.ROWS]
            sec = [[k] for k in range(len(rows))]
            cod = ft.TreeSpace.from_multiplicities(sec, [[(r,)] for r in rows], np.array(p.qdims), 1, [[('r', k)] for k in range(len(rows))],
                                                   [[(k,)] for k in range(len(rows))])
            first = tcases.tree_tensor(self.bb, [rng.standard_normal((r, c)) for r, c in zip(rows, tcases.COLS)], cod, p.dom)
        else:
            legs = [ab.Leg(dc.U1, l.sectors, [int(m) + 1 for m in l.mults], l.sign) for l in p.legs]
            blocks = [rng.standard_normal([int(l.mults[i]) for l, i in zip(legs, r)]) for r in p.inds]
            first = ab.AbelianTensor.from_numpy_blocks(self.bb, dc.U1, legs, blocks, p.inds, 1)
        comps = list(self.template.components) if self.is_sum else [self.template]
        return self.wrap([first] + comps[1:])


class Rig:
    """An ops object under test with its case.  On tensors an operand is the vector itself.  On pools `Vr` and `Vc` are the
    float64 and the complex128 ops objects of the layout (`V` is one of them), so that a check can hand `V` pools of either
    dtype; every pool that is looked at is downloaded whole and its gaps are checked."""

    def __init__(self, case, V, Vr=None, Vc=None):
        self.case, self.V, self.Vr, self.Vc = case, V, Vr, Vc
        self.pool = Vr is not None
        if self.pool:
            assert [tuple(sh) for sh in V.shapes] == case.shapes and Vr.offs == Vc.offs == V.offs
            self.used = np.zeros(V.total, dtype=bool)
            for off, n in zip(V.offs, case.sizes):
                assert not self.used[off:off + n].any()
                self.used[off:off + n] = True

    def enter(self, x, cplx=None):
        if not self.pool:
            return x
        return (self.V if cplx is None else self.Vc if cplx else self.Vr).enter(x)

    def is_complex(self, h):
        return bool(h.is_complex()) if self.pool else bool(np.iscomplexobj(self.case.u(h)))

    def raw(self, h):
        """every byte of an operand: the pool, or the coordinates of a tensor"""
        return (h.cpu().numpy() if self.pool else self.case.u(h)).tobytes()

    def u(self, h):
        """coordinates of an operand; a pool is read where the layout puts the blocks, whatever its support says, and every
        element outside the blocks must be +0.0 byte for byte (the flat reductions rely on it)"""
        if not self.pool:
            return self.case.u(h)
        host = h.cpu().numpy()
        assert host.shape == (self.V.total,)
        gaps = host[~self.used]
        assert gaps.tobytes() == np.zeros(len(gaps), dtype=host.dtype).tobytes(), 'a gap of the pool is not +0.0'
        return np.concatenate([host[off:off + n] for off, n in zip(self.V.offs, self.case.sizes)])

    def y(self, h):
        return self.case.s * self.u(h)

    def apply(self, op, h):
        """op(h) through the public ``matvec`` of the ops object"""
        self.V.H = op
        return self.V.matvec(h)


def _same_bits(got, want):
    """`got` holds the bits of `want`; a real `want` in a complex `got` has the imaginary plane +0.0"""
    got, want = np.asarray(got), np.asarray(want)
    if not np.iscomplexobj(got):
        return not np.iscomplexobj(want) and got.tobytes() == want.tobytes()
    imag = want.imag if np.iscomplexobj(want) else np.zeros(len(want))
    return got.real.tobytes() == np.ascontiguousarray(want.real).tobytes() and got.imag.tobytes() == np.ascontiguousarray(imag).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# enter / leave

def check_enter_leave(rig, rng, cplx):
    """the blocks round-trip bit for bit, full support and a strict subset"""
    V, case = rig.V, rig.case
    for subset in (False, True):
        x, u = case.rand(rng, cplx, subset)
        h = V.enter(x)
        assert _same_bits(case.u(V.leave(h)), u) and _same_bits(rig.u(h), u)


def check_enter_pool(rig, rng):
    """pools: support, views, a real vector in a complex pool, and what ends flat mode.  `rig.V` must be fresh."""
    V, case = rig.V, rig.case
    assert V.support == set()
    x, u = case.rand(rng, V.cplx, subset=True)
    h = V.enter(x)
    assert V.support == set(case.subset)                       # (pool positions are the block numbers of the case)
    back = V.leave(h)
    comps = back.components if case.is_sum else [back]
    assert isinstance(back, DirectSum) == case.is_sum and sum(len(t.blocks) for t in comps) == len(case.subset)
    assert all(b.buf is h for t in comps for b in t.blocks)    # views of the pool, no copy
    assert _same_bits(rig.u(h), u)
    x2, u2 = case.rand(rng, False)
    h2 = V.enter(x2)                                            # a real vector: the real plane of a complex pool
    assert V.support == set(range(len(case.shapes))) and h2.is_complex() == V.cplx and _same_bits(rig.u(h2), u2)
    assert len(h2) == V.total and _same_bits(rig.u(h), u)
    if not V.cplx:
        with pytest.raises(_NeedComplex):
            V.enter(case.rand(rng, True)[0])
    comps = list(case.template.components) if case.is_sum else [case.template]
    wrong = [comps[0], DirectSum(comps + [comps[0]])] + ([DirectSum(comps[:-1])] if len(comps) > 1 else []) if case.is_sum \
        else [DirectSum(comps)]
    for bad in wrong + [case.other_shape(rng)]:
        with pytest.raises(_NotFlat) as err:
            V.enter(bad)
        assert err.type is _NotFlat


# ---------------------------------------------------------------------------------------------------------------------------
# scale / lincomb / combine / _promote

def _check_linear(rig, got, coeffs, us, expect_cplx=None):
    """`got` against sum_k coeffs[k] us[k] elementwise (an accumulator: one more term with the coefficient 1)"""
    k = len(coeffs)
    want = sum(ld(complex(c)) * ld(u) for c, u in zip(coeffs, us))
    size = sum(abs(complex(c)) * np.abs(u) for c, u in zip(coeffs, us))
    err = np.abs(ld(rig.u(got)) - want)
    assert np.all(err <= (k + 3) * EPS * size), float(np.max(err / np.maximum(size, 1e-300)) / EPS)
    if expect_cplx is None:
        expect_cplx = any(np.iscomplexobj(u) for u in us) or any(complex(c).imag != 0.0 for c in coeffs)
    if rig.pool or expect_cplx:        # (numpy makes a complex tensor of a complex coefficient with a zero imaginary part)
        assert rig.is_complex(got) == expect_cplx


def _operands(rig, rng):
    case = rig.case
    xs = {'r1': case.rand(rng, False), 'r2': case.rand(rng, False, True), 'c1': case.rand(rng, True), 'c2': case.rand(rng, True, True)}
    return {k: (rig.enter(x, k[0] == 'c'), u) for k, (x, u) in xs.items()}


def check_scale_lincomb(rig, rng):
    V = rig.V
    ops = _operands(rig, rng)
    for name in ('r1', 'c2'):
        h, u = ops[name]
        for a in (0.75, -1.5, 2.0 - 0.5j, complex(-1.25, 0.0)):
            got = V.scale(a, h)
            _check_linear(rig, got, [a], [u])
            if not isinstance(a, complex):        # one product per component: the values of numpy
                assert np.array_equal(rig.u(got), a * u)
            assert _same_bits(rig.u(h), u)
    for a, b in ((1.0, -0.5), (-1.0, -2.0), (0.5 + 1.0j, 2.0), (1.0, -0.25 - 0.5j), (-0.5 - 1.0j, -2.0 + 0.5j)):
        for p, q in (('r1', 'r2'), ('r1', 'c2'), ('c1', 'r2'), ('c1', 'c2')):
            _check_linear(rig, V.lincomb(a, ops[p][0], b, ops[q][0]), [a, b], [ops[p][1], ops[q][1]])


def check_combine(rig, rng):
    V = rig.V
    ops = _operands(rig, rng)
    H = {k: h for k, (h, _) in ops.items()}
    U = {k: u for k, (_, u) in ops.items()}
    copy = lambda name: V.scale(1.0, H[name])
    # without an accumulator: real, complex coefficients on real operands, mixed operands
    _check_linear(rig, V.combine([0.5, -2.0, 1.25], [H['r1'], H['r2'], H['r1']]), [0.5, -2.0, 1.25], [U['r1'], U['r2'], U['r1']])
    _check_linear(rig, V.combine([0.5 - 1j, 2.0], [H['r1'], H['r2']]), [0.5 - 1j, 2.0], [U['r1'], U['r2']])
    _check_linear(rig, V.combine([complex(0.5, 0.0), 2.0], [H['r1'], H['r2']]), [0.5, 2.0], [U['r1'], U['r2']], False)
    _check_linear(rig, V.combine([-0.5, 2.0 + 1j, 3.0], [H['c1'], H['r2'], H['c2']]), [-0.5, 2.0 + 1j, 3.0], [U['c1'], U['r2'], U['c2']])
    # an accumulator of the result's dtype is updated in place
    for acc_name, coeffs, names in (('c1', [0.5, -1.5 + 2j], ['r1', 'c2']), ('c2', [0.5, -1.5], ['r1', 'r2']), ('r1', [0.5, -1.5], ['r2', 'r1'])):
        acc = copy(acc_name)
        got = V.combine(coeffs, [H[k] for k in names], acc=acc)
        assert got is acc or not rig.pool
        _check_linear(rig, got, [1.0] + coeffs, [U[acc_name]] + [U[k] for k in names])
    # a float64 accumulator under a complex result: a complex pool comes back, the accumulator and its neighbours stay
    for coeffs, names in (([0.5 - 1j, 2.0], ['r2', 'r1']), ([0.5, 2.0], ['c2', 'r2'])):
        before, acc, after = copy('r2'), copy('r1'), copy('r2')
        kept = [rig.raw(t) for t in (before, acc, after)]
        got = V.combine(coeffs, [H[k] for k in names], acc=acc)
        assert got is not acc
        _check_linear(rig, got, [1.0] + coeffs, [U['r1']] + [U[k] for k in names], True)
        assert [rig.raw(t) for t in (before, acc, after)] == kept
    for k, u in U.items():
        assert _same_bits(rig.u(H[k]), u)


def check_promote(rig, rng):
    """pools: the complex128 copy of a float64 pool -- `total` elements, the bits of the real parts, +0.0 imaginary parts"""
    V = rig.V
    for subset in (False, True):
        x, u = rig.case.rand(rng, False, subset)
        h = rig.enter(x, False)
        p = V._promote(h)
        assert p is not h and p.is_complex() and not h.is_complex() and len(p) == V.total
        host = p.cpu().numpy()
        assert host.dtype == np.complex128 and host.real.tobytes() == h.cpu().numpy().tobytes()
        assert host.imag.tobytes() == np.zeros(V.total).tobytes()
        assert _same_bits(rig.u(p), u)
        c = rig.enter(x, True)
        assert V._promote(c) is c


# ---------------------------------------------------------------------------------------------------------------------------
# inner / norm

def check_inner_norm(rig, rng):
    V, case = rig.V, rig.case
    ops = _operands(rig, rng)
    for p, q in (('r1', 'r2'), ('r1', 'c1'), ('c2', 'r1'), ('c2', 'c1')):
        (hv, uv), (hw, uw) = ops[p], ops[q]
        yv, yw = case.s * uv, case.s * uw
        want, tol = ld_vdot(yv, yw), TAU * ld_norm(yv) * ld_norm(yw)
        got, back = V.inner(hv, hw), V.inner(hw, hv)
        if p[0] == q[0] == 'r':
            assert isinstance(got, float) and isinstance(back, float)
        else:
            assert isinstance(got, complex) and isinstance(back, complex)
            assert abs(want.imag) > 1e3 * tol          # (a conjugate on the wrong side is far outside the tolerance)
        assert abs(got - want) <= tol and abs(back - np.conj(want)) <= tol, (p, q, abs(got - want) / tol)
    for name, (h, u) in ops.items():
        want = np.linalg.norm(case.s * u)
        got = V.norm(h)
        assert isinstance(got, float) and abs(got - want) <= TAU * want and abs(got - ld_norm(case.s * u)) <= TAU * want, name


# ---------------------------------------------------------------------------------------------------------------------------
# project_out

def _basis(rig, rng, cplx, m, kind):
    """m basis vectors as (operand, y): 'general' (unit norm, every other one on a subset of the blocks), 'mixed' (the same
    with alternating dtypes) or 'ortho' (orthonormal in y: numpy's QR)"""
    case = rig.case
    out = []
    if kind == 'ortho':
        Q = np.linalg.qr(_random(rng, (case.n, m), cplx))[0] if m else np.zeros((case.n, 0))
        for j in range(m):
            x, u = case.from_y(Q[:, j])
            out.append((rig.enter(x, cplx), case.s * u))
        return out
    for j in range(m):
        c = cplx if kind == 'general' else (j % 2 == 1)
        x, u = case.rand(rng, c, subset=(j % 2 == 1))
        u = u / ld_norm(case.s * u)
        out.append((rig.enter(case.from_u(u, case.subset if j % 2 else None), c), case.s * u))
    return out


def check_project_out(rig, rng, cplx, passes, m, kind):
    """(w - sum_j h_j v_j, h, |w|).  For every basis: the reconstruction w0 = w + sum_j h_j v_j to 1e-12 (|w0| + sum |h_j| |v_j|
    + |w|), the returned norm to 1e-13 relative, the basis unchanged bit for bit, w updated in place on the fused route
    (pools, m <= 64, one dtype).  An orthonormal basis: h = V^H w0 to 1e-13 |w0|, and after two passes |V^H w| <= 1e-13 |w0|.

    A general basis on the fused route, against classical Gram-Schmidt with `passes` passes in extended precision (this is
    what tells two passes from one: h = h1 + h2).  With unit basis vectors, sigma = |V|_2 and tau = 1e-13 the reduction bound:
    |dh1_j| <= tau |w0|; the computed w1 differs from the exact one by -V dh1 + r, |r| <= (m + 2) eps (|w0| + sum |h1_j|);
    so |dh2_j| <= tau |w1| + sigma sqrt(m) tau |w0| + |r|, and |dh_j| <= tau (|w0| + |w1|) + sigma sqrt(m) tau |w0| + |r|."""
    V, case = rig.V, rig.case
    assert m < case.n
    basis = _basis(rig, rng, cplx, m, kind)
    hs, Y = [h for h, _ in basis], (np.array([y for _, y in basis]).T if m else np.zeros((case.n, 0)))
    x0, u0 = case.rand(rng, cplx)
    y0, w = case.s * u0, rig.enter(x0, cplx)
    kept = [rig.raw(h) for h in hs]
    w_out, h, nrm = V.project_out(hs, w, passes)
    fused = rig.pool and m <= V.MAX_BASIS and kind != 'mixed'
    assert (w_out is w) == fused or not rig.pool
    assert [rig.raw(t) for t in hs] == kept
    h = np.asarray(h)
    assert h.shape == (m,)
    yw = rig.y(w_out)
    n0, nw = ld_norm(y0), ld_norm(yw)
    size = n0 + float(np.abs(h) @ np.array([ld_norm(c) for c in Y.T])) + nw
    resid = np.abs(ld(y0) - ld(yw) - ld(Y) @ ld(h))
    assert resid.max() <= 1e-12 * size, float(resid.max() / size)
    assert isinstance(nrm, float) and abs(nrm - nw) <= TAU * nw
    if kind == 'ortho' and m:
        h1 = np.asarray(np.conj(ld(Y)).T @ ld(y0))
        assert np.abs(h - h1).max() <= TAU * n0, float(np.abs(h - h1).max() / n0)
        if passes == 2:
            left = np.abs(np.conj(ld(Y)).T @ ld(yw)).max()
            assert left <= TAU * n0, float(left / n0)
    if kind == 'general' and fused and m:
        wk, hsum, norms, h1abs = ld(y0).astype(np.clongdouble), 0, [], 0.0
        for p in range(passes):
            hp = np.conj(ld(Y)).T @ wk
            h1abs = h1abs or float(np.abs(hp).sum())
            wk = wk - ld(Y) @ hp
            hsum = hsum + hp
            norms.append(float(np.sqrt(np.sum(np.abs(wk) ** 2))))
        bound = TAU * n0
        if passes == 2:
            bound += TAU * norms[0] + np.linalg.norm(Y, 2) * np.sqrt(m) * TAU * n0 + (m + 2) * EPS * (n0 + h1abs)
        err = np.abs(h - hsum).max()
        assert err <= bound, float(err / bound)


# ---------------------------------------------------------------------------------------------------------------------------
# rotate

ROTATIONS = [(5, 5), (6, 3), (3, 5), (4, 35), (40, 35), (65, 2), (3, 0)]      # (m, k)


def check_rotate(rig, rng, cplx, m, k):
    """sum_j Q[j, i] basis_j against Y @ Q.  Pools: k <= min(32, m) rotates in place -- the results ARE basis[:k] and basis[k:]
    keeps its bits --, otherwise the results are fresh pools and every source keeps its bits; m = 65 is the combine route."""
    V, case = rig.V, rig.case
    srcs = [case.rand(rng, cplx, subset=(j % 3 == 1)) for j in range(m)]
    hs = [rig.enter(x, cplx) for x, _ in srcs]
    U = np.array([u for _, u in srcs]).T
    Q = rng.standard_normal((m, k))
    kept = [rig.raw(h) for h in hs]
    out = V.rotate(list(hs), Q)
    assert isinstance(out, list) and len(out) == k
    in_place = rig.pool and 0 < k <= min(V.MAX_ROTATE, m) and m <= V.MAX_BASIS
    if in_place:
        assert all(o is b for o, b in zip(out, hs)) and [rig.raw(t) for t in hs[k:]] == kept[k:]
    else:
        assert not any(o is b for o in out for b in hs) and [rig.raw(t) for t in hs] == kept
    if k == 0:
        return
    want, size = ld(U) @ ld(Q), np.abs(U) @ np.abs(Q)
    for i, o in enumerate(out):
        err = np.abs(ld(rig.u(o)) - want[:, i])
        assert np.all(err <= (m + 2) * EPS * size[:, i]), (i, float(np.max(err / np.maximum(size[:, i], 1e-300)) / EPS))
        assert rig.is_complex(o) == cplx


def check_rotate_errors(rig, rng):
    """pools: mixed dtypes restart on complex pools, a matrix with another row count is an error"""
    V, case = rig.V, rig.case
    x = case.rand(rng, False)[0]
    with pytest.raises(_NeedComplex):
        V.rotate([rig.enter(x, False), rig.enter(x, True)], np.eye(2))
    with pytest.raises(ValueError):
        V.rotate([rig.enter(x), rig.enter(x)], np.ones((3, 2)))
    assert V.rotate([], np.zeros((0, 0))) == []


# ---------------------------------------------------------------------------------------------------------------------------
# orthonormalize (pools)

RCOND = 1e-10


def _cgs2(ys, rcond):
    """numpy restatement of the list orthonormalisation in y: CGS2 against the kept vectors, kept iff the norm is > rcond;
    (norms, kept flags, the remainders before scaling)"""
    done, norms, flags, rests = [], [], [], []
    for y in ys:
        w = ld(y)
        for _ in range(2):
            if done:
                B = np.array(done)
                w = w - (np.conj(B) @ w) @ B
        nrm = float(np.sqrt(np.sum(np.abs(w) ** 2)))
        norms.append(nrm)
        flags.append(nrm > rcond)
        rests.append(w)
        if flags[-1]:
            done.append(w / nrm)
    return np.array(norms), np.array(flags), rests


def orthonormalize_list(case, rng, cplx):
    """[v0, v1, an exact combination of them, v2, one whose remainder is 0.8 rcond, one with 1.2 rcond] as coordinates u, with
    the reference's verdict: the combination's remainder is below 1e-12 of its norm, so numpy alone decides 'dropped' with a
    margin of 100, and the two small ones miss the threshold by 20 % where the rounding of a remainder is 1e-6 of it"""
    us = [case.rand(rng, cplx, subset=(j == 1))[1] for j in range(3)]
    dep = 0.5 * us[0] - 2.0 * us[1]
    us = [us[0], us[1], dep, us[2]]
    for f in (0.8, 1.2):
        u = case.rand(rng, cplx)[1]
        rest = _cgs2([case.s * v for v in us] + [case.s * u], RCOND)[0][-1]
        us.append(u * (f * RCOND / rest))
    norms, flags, _ = _cgs2([case.s * u for u in us], RCOND)
    assert flags.tolist() == [True, True, False, True, False, True]
    assert norms[2] <= 1e-12 * ld_norm(case.s * dep) and abs(norms[4] / RCOND - 0.8) < 1e-3 and abs(norms[5] / RCOND - 1.2) < 1e-3
    return us, norms, flags


def check_orthonormalize(rig, rng, cplx):
    V, case = rig.V, rig.case
    us, norms, flags = orthonormalize_list(case, rng, cplx)
    pools = [rig.enter(case.from_u(u), cplx) for u in us]
    got_norms, got_kept = V.orthonormalize(pools, RCOND)
    assert got_kept.tolist() == flags.tolist()
    ys = [rig.y(p) for p in pools]                              # (the gaps of every pool, dropped ones included)
    for p, keep in zip(pools, flags):
        if not keep:
            host = p.cpu().numpy()
            assert host.tobytes() == np.zeros(V.total, dtype=host.dtype).tobytes()
    assert np.all(np.abs(got_norms[flags] - norms[flags]) <= TAU * norms[flags]), np.abs(got_norms / norms - 1.0)
    K = ld(np.array([y for y, keep in zip(ys, flags) if keep]))
    G = np.conj(K) @ K.T
    m = len(K)
    assert float(np.abs(G - np.eye(m)).max()) <= TAU * m
    assert V.orthonormalize([], RCOND)[0].shape == (0,)
    with pytest.raises(_NeedComplex):
        V.orthonormalize([rig.enter(case.from_u(us[0].real), not V.cplx)], RCOND)


# ---------------------------------------------------------------------------------------------------------------------------
# operator wrappers

def _dense_projected(M, O, project_operator, penalty, y):
    """sparse.ProjectedLinearOperator.matvec on dense vectors: the sequential projection, the operator, the projection
    again, the penalty with the coefficients of the first projection"""
    y = ld(y)
    coef = []
    if project_operator:
        for o in O:
            coef.append(np.sum(np.conj(o) * y))
            y = y - coef[-1] * o
    else:
        coef = [np.sum(np.conj(o) * y) for o in O]
    y = ld(M) @ y
    if project_operator:
        for o in O:
            y = y - np.sum(np.conj(o) * y) * o
    if penalty is not None:
        for o, c in zip(O, coef):
            y = y + penalty * c * o
    return y


def check_apply(rig, rng, cplx):
    """ShiftedLinearOperator, SumLinearOperator and ProjectedLinearOperator (both settings of project_operator, no penalty, a
    real and -- on complex vectors -- a complex one) against the dense formulas in y to 1e-12 |M| |y|"""
    case = rig.case
    H, M = case.H, case.M
    x, u = case.rand(rng, cplx)
    y = case.s * u
    h = rig.enter(x, cplx)
    tol = 1e-12 * np.linalg.norm(M, 2) * ld_norm(y)

    def close(op, want):
        err = float(np.sqrt(np.sum(np.abs(ld(rig.y(rig.apply(op, h))) - want) ** 2)))
        assert err <= tol, err / tol
        assert _same_bits(rig.u(h), u)

    My = ld(M) @ ld(y)
    shifts = [0.5] + ([0.5 - 0.25j] if cplx else [])
    for z in shifts:
        close(sparse.ShiftedLinearOperator(H, z), My + z * ld(y))
    close(sparse.SumLinearOperator(H, [sparse.ShiftedLinearOperator(H, 1.5), H]), 3 * My + 1.5 * ld(y))
    Q = np.linalg.qr(_random(rng, (case.n, 3), cplx))[0]
    ortho, O = [], []
    for j in range(3):
        xo, uo = case.from_y(Q[:, j])
        ortho.append(xo)
        O.append(ld(case.s * uo))
    for project_operator in (True, False):
        for penalty in [None, 2.0] + ([1.5 - 0.5j] if cplx else []):
            op = sparse.ProjectedLinearOperator(sparse.ShiftedLinearOperator(H, 0.5), ortho, project_operator, penalty)
            close(op, _dense_projected(M + 0.5 * np.eye(case.n), O, project_operator, penalty, y))


def check_apply_needs_complex(rig, rng, complex_case):
    """float64 pools: a complex ortho vector, a complex penalty and an operator that returns a complex vector restart the run
    on complex pools.  `complex_case`: the same layout with a complex operator."""
    case = rig.case
    assert not rig.V.cplx
    h = rig.enter(case.rand(rng, False)[0])
    for op in (sparse.ProjectedLinearOperator(case.H, [case.rand(rng, True)[0]]),
               sparse.ProjectedLinearOperator(case.H, [case.rand(rng, False)[0]], penalty=1.0 + 2.0j),
               complex_case.H, sparse.ShiftedLinearOperator(complex_case.H, 0.5)):
        with pytest.raises(_NeedComplex):
            rig.apply(op, h)


def check_three_four(bb, V):
    """the direct sum with the entries 3 and 4 has the norm 5 exactly"""
    h = V.enter(dc.three_four(bb))
    assert V.norm(h) == 5.0 and V.inner(h, h) == 25.0
