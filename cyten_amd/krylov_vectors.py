"""The vectors of the Krylov solvers (:mod:`cyten_amd.krylov`): what ``enter / leave / matvec / norm / inner / scale / lincomb /
combine / project_out / rotate`` are for each kind of vector and each representation.

* On tensors (any backend, a numpy stand-in included): :class:`_TensorOps` for abelian tensors, :class:`_TreeTensorOps` for
  fusion-tree tensors, :class:`_DirectSumOps` for direct sums -- one launch per block LIST, per-block host work.
* On pools (HIP backend only): every vector is ONE contiguous allocation and every operation of the recurrences a single launch
  over it.  :class:`PoolLayout` says where the blocks of a vector lie in its pool -- host arithmetic only, so a CPU test can
  see it -- and :class:`_FlatOps` is the one class with device code.  A fusion-tree vector and a direct sum are a choice of
  layout (:class:`_FlatTreeOps`, :class:`_FlatDirectSumOps`); whether the reductions carry quantum-dimension weights is one
  fact of the layout, a weight table or none.
"""
from __future__ import annotations

import math

import numpy as np

from . import abelian as ab
from . import direct_sum as ds
from . import fusion_tree as ft


class _NotFlat(Exception):
    """The vector left the block structure the flat representation was built for (caught by the solvers' run)."""


class _NeedComplex(_NotFlat):
    """A complex vector met a float64 pool (the operator is complex): the run restarts on complex128 pools."""


def _is_real_scalar(c) -> bool:
    return not isinstance(c, (complex, np.complexfloating)) or complex(c).imag == 0.0


def _negative(c) -> bool:
    """the real part of the scalar has its sign bit set"""
    return bool(np.signbit(complex(c).real))


def _is_tree(t) -> bool:
    return isinstance(t, ft.TreeTensor)


def _mgs(V, basis, w):
    h = []
    for v in basis:
        c = V.inner(v, w)
        h.append(c)
        w = V.lincomb(1.0, w, -c, v)
    return w, np.array(h), V.norm(w)


class _TensorOps:
    """Vector operations of the recurrences on block-sparse tensors (one launch per block LIST, per-block host work)."""

    fused_cgs2 = False    # project_out is ONE pass of modified Gram-Schmidt (a caller that wants two passes runs it twice)

    def __init__(self, bb, H):
        self.bb, self.H = bb, H

    def enter(self, t):
        return t

    def leave(self, w):
        return w

    def matvec(self, w):
        return self.H.matvec(w)

    def norm(self, w):
        return ab.norm(self.bb, w)

    def inner(self, v, w):
        return ab.inner(self.bb, v, w)

    def scale(self, a, w):
        return ab.scale(self.bb, a, w)

    def lincomb(self, a, w, b, v):
        return ab.linear_combination(self.bb, a, w, b, v)

    def combine(self, coeffs, vecs, acc=None):
        """acc + sum_k coeffs[k] vecs[k] (acc None: 0)."""
        out = acc
        for c, v in zip(coeffs, vecs):
            out = self.scale(c, v) if out is None else self.lincomb(1.0, out, c, v)
        return out

    def project_out(self, basis, w, passes=2):
        """(w - sum_j h_j basis_j, h, |w|) by the reference's modified Gram-Schmidt loop (krylov_based.cpp:458-465): one pass,
        each coefficient taken against the vector the earlier ones left (`passes` concerns the fused step of the pools)."""
        return _mgs(self, basis, w)

    def rotate(self, basis, Q):
        """[sum_j Q[j, i] basis_j for every column i of the real m x k matrix `Q`]: k ``combine``, new vectors."""
        Q = np.asarray(Q, dtype=np.float64)
        return [self.combine([float(c) for c in Q[:, i]], basis) for i in range(Q.shape[1])]


class _TreeTensorOps(_TensorOps):
    """:class:`_TensorOps` on fusion-tree vectors (:class:`fusion_tree.TreeTensor`): the inner product and the norm carry the
    quantum dimension of the coupled sector (``FusionTreeBackend::inner`` / ``::norm``); needs nothing of the backend beyond
    what :mod:`cyten_amd.fusion_tree` calls, so it runs on a numpy stand-in."""

    def norm(self, w):
        return ft.norm(self.bb, w.data, w.codomain)

    def inner(self, v, w):
        return ft.inner(self.bb, v.data, w.data, v.codomain, do_dagger=True)

    def scale(self, a, w):
        return w.like(ft.mul(self.bb, a, w.data))

    def lincomb(self, a, w, b, v):
        return w.like(ft.linear_combination(self.bb, a, w.data, b, v.data))


class _DirectSumOps(_TensorOps):
    """:class:`_TensorOps` on direct sums (:class:`direct_sum.DirectSum`): every operation is the componentwise one of
    :mod:`cyten_amd.direct_sum` -- per-component launches; runs on a numpy stand-in."""

    def norm(self, w):
        return ds.norm(self.bb, w)

    def inner(self, v, w):
        return ds.inner(self.bb, v, w)

    def scale(self, a, w):
        return ds.scale(self.bb, a, w)

    def lincomb(self, a, w, b, v):
        return ds.linear_combination(self.bb, a, w, b, v)


# -- where the blocks of a vector lie in its pool (host only) ---------------------------------------------------------------

GRANULE = 256     # elements per entry of a weight table (krylov_vec.hip: a tile of the weighted kernels never sees two weights)


def tree_pool_layout(codomain, domain, granule=GRANULE):
    """The pool of a fusion-tree vector on (codomain, domain): one block per pair of ``ft.common_sectors`` -- every block an
    operator can create -- of shape ``(codomain.block_size(i), domain.block_size(j))``, each starting at a multiple of
    `granule` elements.  Returns (block_inds, shapes, offsets, total, weights): `total` is a multiple of `granule` and
    ``weights[g]`` = ``codomain.qdims[i]`` for every granule g of block (i, j) -- the table the weighted pool reductions read
    (one entry per granule, so a tile of the kernel never sees two weights)."""
    pairs = ft.common_sectors(codomain, domain)
    shapes = [(int(codomain.block_size(i)), int(domain.block_size(j))) for i, j in pairs]
    offs, weights, tot = [], [], 0
    for (i, _), (r, c) in zip(pairs, shapes):
        g = (r * c + granule - 1) // granule
        offs.append(tot)
        tot += g * granule
        weights += [float(codomain.qdims[i])] * g
    return (np.array(pairs, dtype=np.int64).reshape(len(pairs), 2), shapes, offs, tot, np.array(weights, dtype=np.float64))


def _c_strides(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= max(int(s), 1)
    return tuple(reversed(st))


class PoolLayout:
    """Where the blocks of a Krylov vector lie in its pool: numpy and arithmetic only, no device, no allocation.

    `template`: an abelian tensor, a fusion-tree tensor or a direct sum of them; a tensor is the one-component case, and its
    layout is that of ``DirectSum([tensor])``.  The pool holds the segments of the components one after the other, each with
    the layout it has alone:

    * an abelian segment lies over ``AbelianTensor.allowed_block_inds`` -- every block the charge rule allows, what an
      operator can create at most -- its blocks at multiples of 32 elements (`block_inds`: another block table, for a single
      abelian tensor);
    * a tree segment is :func:`tree_pool_layout`.

    Without a tree component there are no weights and the unweighted reductions run over the whole range.  With one, every
    segment is padded to a multiple of 256 elements and the granules of abelian segments get the weight 1.0, so that ONE
    weighted launch covers the range.  Gaps are zero in a pool, hence reductions over the flat range are exact.

    ``tables[i]`` / ``first[i]``: the block table of component i and the position of its first block in ``shapes`` /
    ``strides`` / ``offs`` (one entry per block of the pool, in elements); ``total``: the length of the pool; ``weights``: one
    entry per granule, empty if not ``weighted``."""

    def __init__(self, template, block_inds=None):
        self.is_sum = isinstance(template, ds.DirectSum)
        self.components = list(template.components) if self.is_sum else [template]
        self.weighted = any(_is_tree(c) for c in self.components)
        align = GRANULE if self.weighted else 32
        self.tables, self.first, self.shapes, self.offs, weights, tot = [], [], [], [], [], 0
        for c in self.components:
            if _is_tree(c):
                inds, shapes, offs, n, w = tree_pool_layout(c.codomain, c.domain, GRANULE)
            else:
                inds = ab.AbelianTensor.allowed_block_inds(c.symmetry, c.legs) if block_inds is None or self.is_sum else block_inds
                shapes = [c.block_shape(r) for r in inds]
                offs, n = [], 0
                for sh in shapes:
                    offs.append(n)
                    n += (math.prod(sh) + 31) // 32 * 32
                n = (n + align - 1) // align * align
                w = [1.0] * (n // GRANULE) if self.weighted else []
            self.tables.append(inds)
            self.first.append(len(self.offs))
            self.offs += [tot + o for o in offs]
            self.shapes += list(shapes)
            weights += list(w)
            tot += n
        self.total = tot
        self.strides = [_c_strides(sh) for sh in self.shapes]
        self.weights = np.array(weights, dtype=np.float64)
        self._keys = [t.tobytes() for t in self.tables]
        self._index = [None] * len(self.tables)    # block row -> position, built only if a tensor has fewer blocks than the pool

    def parts(self, x):
        """the tensors of the vector `x`, one per component (_NotFlat: not a vector of this layout's kind or length)"""
        if not self.is_sum:
            if isinstance(x, ds.DirectSum):
                raise _NotFlat()
            return [x]
        if not isinstance(x, ds.DirectSum) or len(x) != len(self.components):
            raise _NotFlat()
        return list(x.components)

    def positions(self, x, i=None):
        """Pool positions of the blocks of the vector `x`, in the order it holds them (`i`: `x` is a tensor of component i).
        A tensor may hold fewer blocks than its segment (the missing ones are zero); _NotFlat: a block the pool does not have."""
        if i is None:
            return [p for k, t in enumerate(self.parts(x)) for p in self.positions(t, k)]
        first, rows = self.first[i], x.block_inds
        if rows.tobytes() == self._keys[i]:
            return list(range(first, first + len(self.tables[i])))
        if self._index[i] is None:
            self._index[i] = {tuple(r): first + n for n, r in enumerate(self.tables[i].tolist())}
        try:
            return [self._index[i][tuple(r)] for r in rows.tolist()]
        except KeyError:
            raise _NotFlat()


# -- the pools --------------------------------------------------------------------------------------------------------------

class _FlatOps:
    """The same operations on Krylov vectors kept as ONE contiguous pool each: the block offsets of
    the structure are computed once (:class:`PoolLayout`), every ``scale / axpy / inner / norm`` of the recurrences is a
    single-descriptor launch over the whole pool -- no per-block host work, one descriptor copy.  The pools are zero between
    blocks, so reductions over the flat range are exact.  Only the operator application sees tensors: its input is a list of
    views into the pool, its output is copied back in one batched launch.

    Pools are float64 while the start vector and the operator are real -- the Lanczos / Arnoldi bases of a real operator
    are real whatever the evolution step delta; only the result assembly ``sum_k c_k v_k`` then has complex coefficients,
    ONE launch of the complex linear combination with real sources.  A complex start vector or operator uses complex128
    pools (interleaved, the same offsets).  Every operation dispatches on the dtype of its pools.

    A layout with a weight table (a fusion-tree component) makes the inner product sum_c d_c <X_c, Y_c>: the pool still holds
    the blocks themselves -- ``leave`` stays views and the operator reads and writes plain blocks -- and the reductions
    (``inner``, ``norm``, the fused Gram-Schmidt step, the multi-dot, ``orthonormalize``) run the weighted entries of
    krylov_vec.hip, which read the quantum dimension of a granule of 256 elements from the table, uploaded ONCE per structure.
    Everything linear (``scale``, ``lincomb``, ``combine``, the multi-axpy, ``rotate``) does not see the weights.

    HIP backend only; anything else uses :class:`_TensorOps`."""

    fused_cgs2 = True     # project_out(passes=2) is the fused CGS2 step

    def __init__(self, bb, H, template, block_inds=None, cplx=False, layout=None):
        """`template`: a vector on the legs of the vectors; `block_inds` (default: the template's): the block table of the
        pool of an abelian tensor -- a superset of the template's when the operator creates blocks the start vector does not
        have; `layout`: the :class:`PoolLayout` to use instead.  `cplx`: the Krylov vectors are complex128 pools."""
        from .block_backend import HipBlock
        from . import _lib
        import ctypes
        self.bb, self.H, self.t, self.cplx = bb, H, template, bool(cplx)
        self._HipBlock, self._lib, self._C = HipBlock, _lib, ctypes
        if layout is None:
            layout = PoolLayout(template, template.block_inds if block_inds is None else block_inds)
        self.layout = L = layout
        self.shapes, self.strides, self.offs, self.total = L.shapes, L.strides, L.offs, L.total
        self.weights, self.weighted = L.weights, L.weighted
        # positions of the pool's blocks that any vector so far holds (the start vector's, plus what the operator produced):
        # the pool is laid out over every charge-allowed block, but the operator only ever sees -- and the result only carries --
        # this support, as the reference's tensors do (krylov_based.cpp works on tensors whose block tables grow the same way)
        self.support = set()
        self._wdev = None
        if self.weighted:
            self._wdev = bb.ctx.empty(max(len(self.weights), 1))
            if len(self.weights):
                bb.ctx.h2d(self._wdev, self.weights)

    @staticmethod
    def usable(bb, t) -> bool:
        return (hasattr(bb, 'ctx') and len(t.blocks) > 0 and not any(b.is_bool for b in t.blocks)
                and type(bb).__name__ != 'DeferredBlockBackend')

    # -- pools
    def _alloc(self, zero, cplx=None):
        bb = self.bb
        cplx = self.cplx if cplx is None else cplx
        buf = bb.ctx.empty(self.total, 'complex128' if cplx else 'float64')
        if zero:
            bb.ctx.sync_stream()
            self._lib.check(bb.lib.cyb_memset(bb.ctx.handle, self._C.c_void_p(buf.data_ptr()), 0, buf.element_size() * self.total))
        return buf

    def _views(self, buf, which):
        bb, mk = self.bb, self._HipBlock._trusted
        return [mk(bb, buf, self.offs[i], self.shapes[i], self.strides[i], True) for i in which]

    def enter(self, x):
        """vector -> pool: one memset + ONE batched copy over the blocks of all components; a real block enters a complex pool
        as its real plane.  Fewer blocks than the pool has are fine (the missing ones are zero); a block outside it, or a
        vector of another kind, ends flat mode."""
        parts = self.layout.parts(x)
        blocks = [b for t in parts for b in t.blocks]
        if not self.cplx and any(b.is_complex for b in blocks):
            raise _NeedComplex()
        buf = self._alloc(True)
        pos = self.layout.positions(x)
        views = self._views(buf, pos)
        if any(v.shape != tuple(b.shape) for v, b in zip(views, blocks)):
            raise _NotFlat()
        self.support.update(pos)
        if views:
            self.bb.copy_many([(v if b.is_complex or not self.cplx else self.bb._plane(v, 0), b) for v, b in zip(views, blocks)])
        return buf

    def leave(self, buf):
        """pool -> vector: every component a tensor of views into the pool over the support (no copy, no allocation); a direct
        sum of them if the template is one"""
        L, comps = self.layout, []
        for t, table, first in zip(L.components, L.tables, L.first):
            idx = [p for p in range(first, first + len(table)) if p in self.support]   # (positions ascend with the block table)
            rows, views = table[[p - first for p in idx]], self._views(buf, idx)
            if _is_tree(t):
                comps.append(t.like(ft.FusionTreeData(rows, views)))
            else:
                comps.append(ab.AbelianTensor(t.symmetry, t.legs, views, rows, t.num_codomain, t.labels))
        return ds.DirectSum(comps) if L.is_sum else comps[0]

    def matvec(self, buf):
        return self._apply(self.H, buf)

    def _apply(self, op, buf):
        """op(buf) on the pools.  The wrappers of cyten_amd.sparse do their vector work here: a shift is one axpby, a sum
        one combine, a projection runs on the device with its coefficients kept there (no host synchronisation); anything
        else sees tensors."""
        from . import sparse
        if isinstance(op, sparse.ShiftedLinearOperator):
            return self.lincomb(1.0, self._apply(op.original_operator, buf), sparse._plain(op.shift), buf)
        if isinstance(op, sparse.SumLinearOperator):
            terms = [self._apply(o, buf) for o in [op.original_operator] + op.more_operators]
            return self.combine([1.0] * len(terms), terms)
        if isinstance(op, sparse.ProjectedLinearOperator):
            return self._projected(op, buf)
        if type(op) is sparse.LinearOperatorWrapper:
            return self._apply(op.original_operator, buf)
        return self.enter(op.matvec(self.leave(buf)))

    def _ortho_pools(self, op):
        """The ortho vectors of a projected operator as pools of this run (entered once)."""
        if not hasattr(self, '_ortho'):
            self._ortho = {}
        got = self._ortho.get(id(op))
        if got is None or got[0] is not op:
            got = (op, [self.enter(o) for o in op.ortho_vecs])
            self._ortho[id(op)] = got
        return got[1]

    def _projected(self, op, buf):
        """The sequential projection of sparse.cpp:294-327 on the pools: every coefficient stays in device memory, each
        projection is one m = 1 Gram-Schmidt launch sequence in the reference's order, the penalty one multi-axpy per vector
        (m = 1: the reference's order) or, for project_operator=False, one multi-dot and one multi-axpy over all of them."""
        O = self._ortho_pools(op)
        cplx = self.cplx
        if any(o.is_complex() != cplx for o in O) or buf.is_complex() != cplx:
            raise _NeedComplex()
        m, stride = len(O), (3 if cplx else 2)
        coef = self.bb.ctx.empty(max(m, 1) * stride)
        res = self.scale(1.0, buf)
        if op.project_operator:
            for j, o in enumerate(O):
                self._gs([o], res, 1, coef, j * stride)
        elif op.penalty is not None and m:
            self._multi('dot', O, res, coef)
        res = self._apply(op.original_operator, res)
        if res.is_complex() != cplx:
            raise _NeedComplex()
        if op.project_operator:
            scratch = self.bb.ctx.empty(stride)
            for o in O:
                self._gs([o], res, 1, scratch, 0)
        if op.penalty is not None and m:
            if not cplx and op.penalty.imag != 0.0:
                raise _NeedComplex()
            p = op.penalty if cplx else op.penalty.real
            if op.project_operator:
                for j, o in enumerate(O):
                    self._multi('axpy', [o], res, coef, j * stride, p)
            else:
                self._multi('axpy', O, res, coef, 0, p)
        return res

    # -- projections against a basis (krylov_vec.hip: cyb_gram_schmidt / cyb_multi_dot / cyb_multi_axpy)
    MAX_BASIS = 64

    def _ptrs(self, basis):
        return (self._C.c_void_p * max(len(basis), 1))(*[v.data_ptr() for v in basis])

    def _weights_ptr(self):
        """the granule table of the weighted entries (None: the unweighted entries run)"""
        return self._C.c_void_p(self._wdev.data_ptr()) if self.weighted else None

    def _reduce(self, name, cplx, *args):
        """One call of the reduction entry `name` on pools of the given dtype: its ``_weighted_`` form, which takes the granule
        table in front of the output argument, if this pool has one -- the ONE place that decides it."""
        bb, wp = self.bb, self._weights_ptr()
        if wp is not None:
            name, args = name + '_weighted', args[:-1] + (wp, args[-1])
        bb.ctx.sync_stream()
        self._lib.check(getattr(bb.lib, name + ('_c128' if cplx else '_f64'))(bb.ctx.handle, *args))

    def _gs(self, basis, w, passes, out, off=0):
        C = self._C
        self._reduce('cyb_gram_schmidt', w.is_complex(), self._ptrs(basis), len(basis), C.c_void_p(w.data_ptr()), self.total,
                     int(passes), C.c_void_p(out.data_ptr() + 8 * off))

    def _multi(self, kind, basis, w, h, off=0, alpha=1.0):
        bb, C = self.bb, self._C
        cp = w.is_complex()
        hp = C.c_void_p(h.data_ptr() + 8 * off)
        if kind == 'dot':
            return self._reduce('cyb_multi_dot', cp, self._ptrs(basis), len(basis), C.c_void_p(w.data_ptr()), self.total, hp)
        bb.ctx.sync_stream()
        if cp:
            a = complex(alpha)
            self._lib.check(bb.lib.cyb_multi_axpy_c128(bb.ctx.handle, self._ptrs(basis), len(basis), hp, a.real, a.imag,
                                                       C.c_void_p(w.data_ptr()), self.total))
        else:
            self._lib.check(bb.lib.cyb_multi_axpy_f64(bb.ctx.handle, self._ptrs(basis), len(basis), hp, float(np.real(alpha)),
                                                      C.c_void_p(w.data_ptr()), self.total))

    def orthonormalize(self, pools, rcond):
        """The list `pools` (at most MAX_BASIS, of the dtype of this run) orthonormalised in place by ONE library call
        (krylov_vec.hip: cyb_orthonormalize_*): CGS2 of each against the earlier ones, then scaled by 1 / norm if the norm is
        > rcond, else overwritten with zeros -- no host wait between the steps.  ONE download at the end: (norms, kept)."""
        bb, m = self.bb, len(pools)
        if any(p.is_complex() != self.cplx for p in pools):
            raise _NeedComplex()
        if m == 0 or self.total == 0:
            return np.zeros(0), np.zeros(0, dtype=bool)
        out = bb.ctx.empty(2 * m)
        self._reduce('cyb_orthonormalize', self.cplx, self._ptrs(pools), m, self.total, float(rcond), self._C.c_void_p(out.data_ptr()))
        r = bb.ctx.d2h(out, 2 * m, np.float64)
        return r[:m].copy(), r[m:] != 0.0

    def project_out(self, basis, w, passes=2):
        """(w - V h, h, |w - V h|) with h = V^H w: ONE fused classical Gram-Schmidt call (passes=2: CGS2, h summed over the
        passes) that updates w in place, and ONE device-to-host copy of the m coefficients and the norm.  A basis of mixed
        dtypes or longer than the kernel takes runs the modified Gram-Schmidt loop of _TensorOps."""
        m = len(basis)
        cplx = w.is_complex()
        if m > self.MAX_BASIS or any(v.is_complex() != cplx for v in basis):
            return _mgs(self, basis, w)
        k = 2 if cplx else 1
        out = self.bb.ctx.empty(k * m + 1)
        self._gs(basis, w, passes, out)
        r = self.bb.ctx.d2h(out, k * m + 1, np.float64)
        h = (r[0:2 * m:2] + 1j * r[1:2 * m:2]) if cplx else r[:m].copy()
        return w, h, float(r[k * m])

    MAX_ROTATE = 32    # columns of one cyb_basis_rotate_f64 call

    def rotate(self, basis, Q):
        """The pools sum_j Q[j, i] basis_j for every column i of the real m x k matrix `Q` (the restart of
        :class:`krylov.LanczosEigenpairs`) by ONE cyb_basis_rotate_f64 call IN PLACE: the results replace basis[0 .. k-1] (which
        are returned), basis[k:] is untouched; nothing is downloaded.  The matrix is real, so a complex pool is rotated as its
        2 * total doubles.  More than MAX_ROTATE columns (or more columns than pools): chunks of MAX_ROTATE columns, each one
        call of the same entry that writes to fresh pools.  A basis longer than the kernel takes runs k ``combine``."""
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        m, k = Q.shape
        if m != len(basis):
            raise ValueError(f'rotate: {len(basis)} vectors, a matrix of {m} rows')
        if k == 0:
            return []
        cplx = basis[0].is_complex()
        if any(v.is_complex() != cplx for v in basis):
            raise _NeedComplex()
        if m > self.MAX_BASIS:
            return _TensorOps.rotate(self, basis, Q)
        words = (2 if cplx else 1) * self.total
        in_place = k <= min(self.MAX_ROTATE, m)
        out = []
        for c0 in range(0, k, self.MAX_ROTATE):
            Qc = Q if in_place else np.ascontiguousarray(Q[:, c0:c0 + self.MAX_ROTATE])
            dst = list(basis[:k]) if in_place else [self._alloc(False, cplx) for _ in range(Qc.shape[1])]
            self._rotate_call(basis, dst, Qc, words)
            out += dst
        return out

    def _rotate_call(self, src, dst, Q, words):
        bb, C = self.bb, self._C
        bb.ctx.sync_stream()
        self._lib.check(bb.lib.cyb_basis_rotate_f64(bb.ctx.handle, self._ptrs(src), len(src), self._ptrs(dst), len(dst),
                                                    Q.ctypes.data_as(C.c_void_p), words))

    # -- BLAS-1 over the flat range
    def _desc(self, x, y, out, n=None):
        arr = np.zeros(1, dtype=self._lib.VEC_DTYPE)
        arr['x'][0] = x.data_ptr()
        arr['y'][0] = y.data_ptr() if y is not None else 0
        arr['out'][0] = out.data_ptr() if out is not None else 0
        arr['n'][0] = self.total if n is None else n
        return arr

    def _call(self, name, arr, *args):
        bb = self.bb
        bb.ctx.sync_stream()
        self._lib.check(getattr(bb.lib, name)(bb.ctx.handle, arr.ctypes.data_as(self._C.POINTER(self._lib.VecDesc)), 1, *args))

    def combine(self, coeffs, vecs, acc=None, cplx=None):
        """acc + sum_k coeffs[k] vecs[k] in ONE launch over the flat range (the result assembly of the solvers).  Complex
        coefficients or pools: the complex linear combination, float64 pools read as real sources (`src_real`), the
        result a complex pool; `acc` of the result's dtype is updated in place, a float64 `acc` under a complex result is
        left alone (the sum goes to its complex copy).  Real throughout: the float64 form.  `cplx` True: the complex form
        whatever the coefficients and pools are."""
        bb, L = self.bb, self._lib
        cplx = bool(cplx or any(v.is_complex() for v in vecs) or not all(_is_real_scalar(c) for c in coeffs)
                    or (acc is not None and acc.is_complex()))
        if acc is not None and acc.is_complex() != cplx:
            acc = self._promote(acc)
        out = acc if acc is not None else self._alloc(False, cplx)
        desc = np.zeros(1, dtype=L.LINCOMB_DTYPE)
        desc['dst'][0] = out.data_ptr()
        desc['ndim'][0] = 1
        desc['accumulate'][0] = 1 if acc is not None else 0
        desc['term_begin'][0], desc['term_end'][0] = 0, len(vecs)
        desc['shape'][0, 0] = self.total
        desc['dst_strides'][0, 0] = 1
        terms = np.zeros(len(vecs), dtype=L.LINTERM_C128_DTYPE if cplx else L.LINTERM_DTYPE)
        terms['src'] = [v.data_ptr() for v in vecs]
        terms['src_strides'][:, 0] = 1
        if cplx:
            cs = [complex(c) for c in coeffs]
            terms['coeff_re'] = [c.real for c in cs]
            terms['coeff_im'] = [c.imag for c in cs]
            terms['src_real'] = [0 if v.is_complex() else 1 for v in vecs]
        else:
            terms['coeff'] = [float(np.real(c)) for c in coeffs]
        bb.ctx.sync_stream()
        fn = bb.lib.cyb_lincomb_strided_batched_c128 if cplx else bb.lib.cyb_lincomb_strided_batched_f64
        T = L.LincombTermC128 if cplx else L.LincombTerm
        self._lib.check(fn(bb.ctx.handle, desc.ctypes.data_as(self._C.POINTER(L.LincombDesc)), 1,
                           terms.ctypes.data_as(self._C.POINTER(T)), len(vecs)))
        return out

    def _promote(self, w):
        """complex128 copy of a float64 pool (a complex pool: itself): ONE launch of the complex linear combination with a
        real source, (1 + 0i) * (x + 0i) added to +0.0 -- the real parts are those of `w`, the imaginary parts +0.0.  The
        complex form is asked for by name: the coefficient 1 alone is a real scalar and would give a float64 pool."""
        return w if w.is_complex() else self.combine([1.0], [w], cplx=True)

    def lincomb(self, a, w, b, v):
        # (two coefficients with negative real parts: a * 0 + b * 0 is -0.0 in the axpby kernels, and the gaps of a pool stay
        # +0.0; the linear combination adds its terms to +0.0)
        if (w.is_complex() != v.is_complex() or (not w.is_complex() and not (_is_real_scalar(a) and _is_real_scalar(b)))
                or (_negative(a) and _negative(b))):
            return self.combine([a, b], [w, v])
        out = self._alloc(False, w.is_complex())
        if w.is_complex():
            a, b = complex(a), complex(b)
            self._call('cyb_axpby_batched_c128', self._desc(w, v, out), a.real, a.imag, b.real, b.imag)
        else:
            self._call('cyb_axpby_batched_f64', self._desc(w, v, out), float(np.real(a)), float(np.real(b)))
        return out

    def scale(self, a, w):
        if not w.is_complex() and not _is_real_scalar(a):
            return self.combine([a], [w])
        out = self._alloc(False, w.is_complex())
        # a negative real part: a * 0 is -0.0, so the kernel adds 0 * w -- the same values, and the gaps stay +0.0
        y = w if _negative(a) else None
        if w.is_complex():
            a = complex(a)
            self._call('cyb_axpby_batched_c128', self._desc(w, y, out), a.real, a.imag, 0.0, 0.0)
        else:
            self._call('cyb_axpby_batched_f64', self._desc(w, y, out), float(np.real(a)), 0.0)
        return out

    def inner(self, v, w):
        """<v, w> = sum conj(v) w, with weights sum_c d_c sum conj(v_c) w_c: a float on float64 pools, a complex number
        otherwise.  Unweighted: cyb_dot_batched_*; weighted: the weighted multi-dot with the basis [v]."""
        bb = self.bb
        cplx = v.is_complex() or w.is_complex()
        if cplx:
            v = v if v.is_complex() else self._promote(v)
            w = w if w.is_complex() else self._promote(w)
        k = 2 if cplx else 1
        res = bb.ctx.empty(k)
        if self.weighted:
            self._multi('dot', [v], w, res)
        else:
            self._call('cyb_dot_batched_c128' if cplx else 'cyb_dot_batched_f64', self._desc(v, w, None), self._C.c_void_p(res.data_ptr()))
        r = bb.ctx.d2h(res, k, np.float64)
        return complex(float(r[0]), float(r[1])) if cplx else float(r[0])

    def norm(self, w):
        if self.weighted:
            return float(np.sqrt(max(np.real(self.inner(w, w)), 0.0)))
        if not w.is_complex():
            return float(np.sqrt(self.inner(w, w)))
        # the float64 reduction over the interleaved storage: sum re^2 + im^2
        bb = self.bb
        res = bb.ctx.empty(1)
        self._call('cyb_dot_batched_f64', self._desc(w, w, None, 2 * self.total), self._C.c_void_p(res.data_ptr()))
        return float(np.sqrt(bb.ctx.d2h(res, 1, np.float64)[0]))


class _FlatTreeOps(_FlatOps):
    """:class:`_FlatOps` on the pool of one fusion-tree vector (:func:`tree_pool_layout`): a weighted layout, DESIGN.md 4.14."""

    def __init__(self, bb, H, template, cplx=False):
        super().__init__(bb, H, template, cplx=cplx, layout=PoolLayout(template))

    @staticmethod
    def usable(bb, t) -> bool:
        # (an empty pool -- no pair of common sectors with a non-empty block -- is not: asked of the spaces, not of a layout)
        return _FlatOps.usable(bb, t) and any(int(t.codomain.block_size(i)) * int(t.domain.block_size(j)) > 0
                                              for i, j in ft.common_sectors(t.codomain, t.domain))


class _FlatDirectSumOps(_FlatOps):
    """:class:`_FlatOps` on the pool of a direct sum: the pools of its components -- each with the layout it
    has alone -- one after the other in ONE allocation, so that every recurrence, the fused CGS2 step and the projected matvec
    are the single launches they are for one tensor.  With ONE component the pool is byte for byte that of the tensor.  The
    support is tracked per block, hence per component."""

    def __init__(self, bb, H, template, cplx=False):
        super().__init__(bb, H, template, cplx=cplx, layout=PoolLayout(template))


def _vector_ops(bb, H, template, mode):
    """The vector operations of a run on vectors like `template`: pools (`mode` False / True: float64 / complex128) or
    tensors (`mode` None); abelian, fusion-tree or direct-sum by the type of the template."""
    if isinstance(template, ds.DirectSum):
        return _FlatDirectSumOps(bb, H, template, mode) if mode is not None else _DirectSumOps(bb, H)
    if _is_tree(template):
        return _FlatTreeOps(bb, H, template, mode) if mode is not None else _TreeTensorOps(bb, H)
    if mode is None:
        return _TensorOps(bb, H)
    # pool structure: every block the charge rule allows on these legs (what an operator can create at most)
    return _FlatOps(bb, H, template, ab.AbelianTensor.allowed_block_inds(template.symmetry, template.legs), mode)


def _flat_usable(bb, t) -> bool:
    return _FlatTreeOps.usable(bb, t) if _is_tree(t) else _FlatOps.usable(bb, t)
