"""Linear-operator wrappers of the Krylov solvers (include/cyten/tensors/sparse.h:66-128, src/tensors/sparse.cpp:188-344).

* :class:`LinearOperatorWrapper` -- forwards to ``original_operator``; ``unwrapped()`` peels wrappers off.
* :class:`SumLinearOperator` -- ``op + sum(more_operators)`` (sparse.cpp:196-241).
* :class:`ShiftedLinearOperator` -- ``op + shift`` (sparse.cpp:243-275); complex when the shift is.
* :class:`ProjectedLinearOperator` -- ``P op P + penalty (1 - P)`` with ``P = 1 - sum_o |o><o|``, or ``op + penalty (1 - P)``
  with ``project_operator=False`` (sparse.cpp:277-344).  The projection is the reference's SEQUENTIAL one: each ortho vector
  is removed from the current vector in turn.  For orthonormal ortho vectors that is the projector above; for others it is
  what the reference computes (its docstring, py_sparse.cpp:322-324, promises a Gram-Schmidt the code does not do).

* :class:`TensorLinearOperator` -- a two-leg abelian tensor acting on one-leg tensors (sparse.cpp:68-140).
* :class:`DirectSumLinearOperator` -- the block-diagonal operator on a ``direct_sum.DirectSum`` (sparse.cpp:346-418).
* :func:`gram_schmidt` -- a list of vectors orthonormalised, the dependent ones dropped (sparse.cpp:420-436).

Every wrapper acts on block-sparse tensors -- abelian ones or fusion-tree ones (``fusion_tree.TreeTensor``, whose inner product
carries the quantum dimensions) -- and on direct sums of them (``direct_sum.DirectSum``) through ``.matvec(tensor)`` with the block backend of the wrapped operator (or the
``bb`` given), exposes ``is_complex`` as the solvers expect and has ``adjoint()`` where the wrapped operators have one.  On
flat Krylov pools the solvers do not call these ``matvec``s: ``krylov._FlatOps`` recognises the wrappers and does their
vector work on the pools.
"""
from __future__ import annotations

import numpy as np

from . import abelian as ab
from . import direct_sum as ds
from .direct_sum import vectors_compatible as _compatible


def _is_complex_op(op) -> bool:
    return bool(getattr(op, 'is_complex', False))


def _is_complex_tensor(t) -> bool:
    return any(np.iscomplexobj(b) if isinstance(b, np.ndarray) else bool(b.is_complex) for b in t.blocks)


def _plain(c):
    """A complex number with a zero imaginary part as a float (keeps float64 vectors real)."""
    c = complex(c)
    return c.real if c.imag == 0.0 else c


class LinearOperatorWrapper:
    """Base class of the wrappers: forwards to ``original_operator`` (sparse.cpp:160-186)."""

    def __init__(self, original_operator, bb=None):
        self.original_operator = original_operator
        self.bb = bb if bb is not None else getattr(original_operator, 'bb', None)

    @property
    def is_complex(self) -> bool:
        return _is_complex_op(self.original_operator)

    def unwrapped(self, recursive: bool = True):
        op = self.original_operator
        while recursive and isinstance(op, LinearOperatorWrapper):
            op = op.original_operator
        return op

    def matvec(self, vec):
        return self.original_operator.matvec(vec)

    def adjoint(self):
        return LinearOperatorWrapper(self.original_operator.adjoint(), self.bb)


class SumLinearOperator(LinearOperatorWrapper):
    """``original_operator + sum(more_operators)``."""

    def __init__(self, original_operator, more_operators=(), bb=None):
        super().__init__(original_operator, bb)
        self.more_operators = list(more_operators)

    @property
    def is_complex(self) -> bool:
        return _is_complex_op(self.original_operator) or any(_is_complex_op(op) for op in self.more_operators)

    def matvec(self, vec):
        res = self.original_operator.matvec(vec)
        for op in self.more_operators:
            res = ds.vector_lincomb(self.bb, 1.0, op.matvec(vec), 1.0, res)
        return res

    def adjoint(self):
        return SumLinearOperator(self.original_operator.adjoint(), [op.adjoint() for op in self.more_operators], self.bb)


class ShiftedLinearOperator(LinearOperatorWrapper):
    """``original_operator + shift * 1``; complex if ``shift.imag != 0``."""

    def __init__(self, original_operator, shift, bb=None):
        super().__init__(original_operator, bb)
        self.shift = complex(shift)

    @property
    def is_complex(self) -> bool:
        return _is_complex_op(self.original_operator) or self.shift.imag != 0.0

    def matvec(self, vec):
        res = self.original_operator.matvec(vec)
        return ds.vector_lincomb(self.bb, _plain(self.shift), vec, 1.0, res)

    def adjoint(self):
        return ShiftedLinearOperator(self.original_operator.adjoint(), self.shift.conjugate(), self.bb)


class ProjectedLinearOperator(LinearOperatorWrapper):
    """``P H P + penalty (1 - P)`` (``project_operator=True``) or ``H + penalty (1 - P)``, ``P = 1 - sum_o |o><o|``;
    ``penalty=None`` means 0.  The coefficients of the penalty term are those the sequential projection of the input
    produced (sparse.cpp:294-327)."""

    def __init__(self, original_operator, ortho_vecs, project_operator: bool = True, penalty=None, bb=None):
        super().__init__(original_operator, bb)
        self.ortho_vecs = list(ortho_vecs)
        self.project_operator = bool(project_operator)
        self.penalty = None if penalty is None else complex(penalty)
        for v in self.ortho_vecs[1:]:
            if not _compatible(v, self.ortho_vecs[0]):
                raise ValueError('All ortho_vecs must be mutually compatible')

    @property
    def is_complex(self) -> bool:
        return (_is_complex_op(self.original_operator) or any(_is_complex_tensor(v) for v in self.ortho_vecs)
                or (self.penalty is not None and self.penalty.imag != 0.0))

    def with_original(self, op) -> 'ProjectedLinearOperator':
        """The same projection around another operator."""
        return ProjectedLinearOperator(op, self.ortho_vecs, self.project_operator, self.penalty, self.bb)

    def matvec(self, vec):
        bb = self.bb
        res = vec
        coeffs = []
        if self.project_operator:
            for o in self.ortho_vecs:
                c = ds.vector_inner(bb, o, res)
                coeffs.append(c)
                res = ds.vector_lincomb(bb, 1.0, res, _plain(-c), o)
        else:
            coeffs = [ds.vector_inner(bb, o, res) for o in self.ortho_vecs]
        res = self.original_operator.matvec(res)
        if self.project_operator:
            for o in self.ortho_vecs:
                c = ds.vector_inner(bb, o, res)
                res = ds.vector_lincomb(bb, 1.0, res, _plain(-c), o)
        if self.penalty is not None:
            for o, c in zip(self.ortho_vecs, coeffs):
                res = ds.vector_lincomb(bb, 1.0, res, _plain(self.penalty * c), o)
        return res

    def adjoint(self):
        p = None if self.penalty is None else self.penalty.conjugate()
        return ProjectedLinearOperator(self.original_operator.adjoint(), self.ortho_vecs, self.project_operator, p, self.bb)


class TensorLinearOperator:
    """A two-leg abelian tensor as an operator on one-leg tensors (sparse.cpp:68-140): ``matvec(v)`` contracts leg
    `which_leg` of the tensor with the leg of `v`.  The fusion-tree counterpart is a one-step ``krylov.TreeChainOperator``."""

    def __init__(self, bb, tensor, which_leg: int = -1):
        if tensor is None:
            raise ValueError('tensor must not be null')
        if tensor.nlegs != 2:
            raise ValueError('Expected a two-leg tensor')
        if not isinstance(which_leg, (int, np.integer)) or not -2 <= which_leg < 2:
            raise ValueError('which_leg must refer to a single leg')
        self.bb, self.tensor = bb, tensor
        self.which_leg = int(which_leg) % 2
        self.other_leg = 1 - self.which_leg
        if not tensor.legs[self.which_leg].can_contract_with(tensor.legs[self.other_leg]):
            raise ValueError('Expected contractible legs')
        self.vector_legs = [tensor.legs[self.other_leg]]

    @property
    def is_complex(self) -> bool:
        return _is_complex_tensor(self.tensor)

    def matvec(self, vec):
        if not isinstance(vec, ab.AbelianTensor):
            raise ValueError('TensorLinearOperator.matvec expects a Tensor input')
        if vec.nlegs != 1:
            raise ValueError('TensorLinearOperator.matvec expects a single-leg tensor')
        res = ab.tdot(self.bb, self.tensor, vec, [self.which_leg], [0])
        res.num_codomain = vec.num_codomain
        return res

    def to_tensor(self):
        if self.which_leg == 1:
            return self.tensor
        return ab.permute_legs(self.bb, self.tensor, [self.other_leg, self.which_leg])

    def adjoint(self):
        return TensorLinearOperator(self.bb, ab.dagger(self.bb, self.tensor), self.which_leg)


class DirectSumLinearOperator:
    """The block-diagonal operator on a :class:`direct_sum.DirectSum` (sparse.cpp:346-418): component i of the vector goes
    through ``operators[i]``.  On flat pools (``krylov._FlatDirectSumOps``) wrappers around it work on the whole pool; the
    operators inside it, their own wrappers included, see the tensors of their component."""

    def __init__(self, operators, bb=None):
        self.operators = list(operators)
        if not self.operators:
            raise ValueError('DirectSumLinearOperator needs at least one operator')
        for op in self.operators:
            if op is None or not hasattr(op, 'matvec'):
                raise ValueError('DirectSumLinearOperator operators must be objects with a matvec')
        self.bb = bb if bb is not None else next((op.bb for op in self.operators if getattr(op, 'bb', None) is not None), None)

    @property
    def is_complex(self) -> bool:
        return any(_is_complex_op(op) for op in self.operators)

    def matvec(self, vec):
        if not isinstance(vec, ds.DirectSum):
            raise ValueError('DirectSumLinearOperator.matvec expects a DirectSum input')
        if len(vec) != len(self.operators):
            raise ValueError('DirectSumLinearOperator.matvec expects matching component count')
        return ds.DirectSum([op.matvec(c) for op, c in zip(self.operators, vec.components)])

    def to_tensor(self):
        raise NotImplementedError('DirectSumLinearOperator has no single-tensor representation')

    def adjoint(self):
        return DirectSumLinearOperator([op.adjoint() for op in self.operators], self.bb)


def gram_schmidt(bb, vecs, rcond: float = 1e-14):
    """The orthonormal vectors of sparse.cpp:420-436 from a list of pairwise compatible vectors (tensors, tree tensors or
    direct sums): a vector is kept iff the norm of what the earlier kept ones leave of it is ``> rcond`` -- strict and absolute,
    a NaN norm drops it.  How the ortho_vecs of a :class:`ProjectedLinearOperator` are prepared.

    On ``HipBlockBackend`` the list runs on pools in ONE library call (``cyb_orthonormalize_*``): CGS2 per
    vector, dropped vectors zeroed on the device, and one download of the norms and flags at the end; elsewhere it is the
    reference's loop on tensors."""
    vecs = list(vecs)
    for v in vecs[1:]:
        if not _compatible(v, vecs[0]):
            raise ValueError('gram_schmidt: all vectors must be mutually compatible')
    from . import krylov
    if vecs and len(vecs) <= krylov._FlatOps.MAX_BASIS and krylov._flat_usable(bb, vecs[0]):
        try:
            V = krylov._vector_ops(bb, None, vecs[0], any(_is_complex_tensor(v) for v in vecs))
            pools = [V.enter(v) for v in vecs]
            _, kept = V.orthonormalize(pools, rcond)
            return [V.leave(p) for p, k in zip(pools, kept) if k]
        except krylov._NotFlat:
            pass
    res = []
    for v in vecs:
        for o in res:
            v = ds.vector_lincomb(bb, _plain(-complex(ds.vector_inner(bb, o, v))), o, 1.0, v)
        n = ds.vector_norm(bb, v)
        if n > rcond:
            res.append(ds.vector_scale(bb, 1.0 / n, v))
    return res

