"""The Lanczos matvec group of the DMRG inner loop on the grouped device path.

* :class:`HEffective` -- the two-site effective Hamiltonian of the reference's DMRG toycode
  (/root/reference/toycodes/tenpy_toycodes/d_dmrg.py:55-86): ``matvec`` = 4 ``compose`` + 4
  ``permute_legs``.  Every compose is ONE grouped-GEMM launch (plus at most one batched copy that makes
  permuted operands contiguous); the host-side sector matching of a compose is computed once per
  operand structure and reused by all later matvecs (the block tables do not change between Lanczos
  iterations).
* :class:`LanczosGroundState` / :func:`lanczos` -- the reference's Lanczos iteration
  (/root/reference/src/tensors/krylov_based.cpp:803-946, options :276-288): same recurrences,
  same convergence test, same result assembly; ``inner`` / ``norm`` / ``axpy`` run as one launch
  each over the whole block list, the (k+1) x (k+1) tridiagonal problem stays on the host as in the
  reference (numpy.linalg.eigh, :922-946).
* :class:`LanczosEvolution`, :class:`Arnoldi`, :class:`ArnoldiEvolution` -- exp(delta H) psi (the TDVP step) and the
  non-Hermitian eigensolver of the reference (krylov_based.cpp:532-800, 948-1019), on the same flat pools: float64 while the
  operator and the start vector are real, complex128 otherwise.
* :class:`LanczosEigenpairs` / :func:`eigenvectors` -- several eigenpairs of a Hermitian operator by thick-restart Lanczos on one
  bounded basis (the reference: ARPACK through a host array per matvec, sparse.py:410-504): full reorthogonalisation by the fused
  CGS2 call, the restart ONE in-place basis rotation on the pools (krylov_vec.hip: cyb_basis_rotate_f64).
* Every solver takes fusion-tree vectors (:class:`cyten_amd.fusion_tree.TreeTensor`) as well: the recurrences are the same
  code, the vector operations are :class:`_TreeTensorOps` (tensors) or :class:`_FlatTreeOps` (pools whose reductions carry the
  quantum dimension of the coupled sector); :class:`TreeChainOperator` is an operator to apply to them.
* ... and direct sums of both (:class:`cyten_amd.direct_sum.DirectSum`): :class:`_DirectSumOps` on tensors,
  :class:`_FlatDirectSumOps` on pools that hold the components' pools one after the other.

Leg orders used here (signs: + ket-like, - dual):
    theta [vL, p0, p1, vR]
    LP    [vL', wL, vL*]          W1 [p0', wC, p0*, wL*]
    W2    [p1', wR, p1*, wC*]     RP [wR*, vR*, vR']
``compose(a, b, k)`` contracts the last k legs of a with the first k legs of b, a's in reversed order.
"""
from __future__ import annotations

import numpy as np

from . import abelian as ab
from . import direct_sum as ds
from . import fusion_tree as ft


def _is_complex_block(b) -> bool:
    return np.iscomplexobj(b) if isinstance(b, np.ndarray) else bool(b.is_complex)


class HEffective:
    """theta' = H_eff theta for a two-site DMRG update (d_dmrg.py:74-86)."""

    def __init__(self, bb, LP, W1, W2, RP, replay: bool = True, cache: dict | None = None):
        """`cache`: a dict the caller keeps across operators (a DMRG run keeps one for all bonds and sweeps).  The
        recorded launch sequences are relocatable in ALL five operands (environments, MPO tensors and the vector), so a
        bond whose block layouts have been seen before -- every bond from the second sweep on, once the sector
        structure has settled -- is served by replays only."""
        self.bb, self.LP, self.W1, self.W2, self.RP = bb, LP, W1, W2, RP
        self._plans = {}
        self.flops_per_matvec = None
        # recorded launch sequences, one per block layout of the operands (cyten_amd/replay.py); only a backend that
        # issues C-ABI launches can be recorded
        self._recordings = (cache if cache is not None else {}) if (replay and hasattr(bb, 'ctx')) else None
        self._op_layout = None
        self._op_layout_rc = None
        self._RP_t = None
        self.is_complex = any(_is_complex_block(b) for t in (LP, W1, W2, RP) for b in t.blocks)
        self.n_replayed = 0
        self.n_recorded = 0

    def _real_on_complex(self, theta) -> bool:
        """A complex vector under a real operator: every compose runs as real A x complex B (`_real_complex_gemm`)."""
        return not self.is_complex and any(_is_complex_block(b) for b in theta.blocks)

    def _rp_t(self):
        """RP with its legs in the order [vR', vR*, wR*], contiguous: the last compose of a complex vector takes RP as
        its (real) A operand.  Made ONCE; it is part of the fixed operator layout of the recordings, so a shared cache
        relocates it like the other operands."""
        if self._RP_t is None:
            t = ab.permute_legs(self.bb, self.RP, [2, 1, 0])
            self._RP_t = ab.AbelianTensor(t.symmetry, t.legs, self.bb.contiguous_many(t.blocks), t.block_inds, t.num_codomain)
        return self._RP_t

    def _compose(self, tag, a, b, k):
        key = (tag, a.block_inds.tobytes(), b.block_inds.tobytes())
        plan = self._plans.get(key)
        if plan is None:
            plan = ab.compose_plan(a, b, k)
            self._plans[key] = plan
        na_keep = a.nlegs - k
        if not plan.pairs:
            return ab.AbelianTensor(a.symmetry, plan.legs, [], plan.res_block_inds, na_keep), 0.0
        a2, b2 = ab._compose_operands(self.bb, a, b, k, plan)
        outs = self.bb.matrix_dot_grouped([[(a2[i], b2[j]) for i, j in g] for g in plan.pairs])
        blocks = [self.bb.reshape(o, shp) for o, shp in zip(outs, plan.res_shapes)]
        return ab.AbelianTensor(a.symmetry, plan.legs, blocks, plan.res_block_inds, na_keep), plan.flops

    def matvec(self, theta):
        """H_eff theta.  The first application to an input of a given block layout runs the ordinary path while its
        allocations and launches are recorded; later applications replay them with the pointers rewritten."""
        if self._recordings is None:
            return self._matvec(theta)
        from .replay import apply_recorded, tensor_layout
        if self._real_on_complex(theta):
            if self._op_layout_rc is None:
                bufs, sizes = [], {}
                sig = tensor_layout([self.LP, self.W1, self.W2, self._rp_t()], bufs, sizes)
                self._op_layout_rc = (sig, bufs, sizes)
            tag, fixed = 'heff_rc', self._op_layout_rc
        else:
            if self._op_layout is None:
                bufs, sizes = [], {}
                sig = tensor_layout([self.LP, self.W1, self.W2, self.RP], bufs, sizes)
                self._op_layout = (sig, bufs, sizes)
            tag, fixed = 'heff', self._op_layout
        out, how, rec = apply_recorded(self.bb, self._recordings, tag, lambda: self._matvec(theta), [theta], fixed=fixed)
        if how == 'recorded':
            self.n_recorded += 1
            rec.flops = self.flops_per_matvec
        elif how == 'replayed':
            self.n_replayed += 1
            self.flops_per_matvec = rec.flops
        return out

    def _matvec(self, theta):
        bb = self.bb
        flops = 0.0
        x, f = self._compose('LP', self.LP, theta, 1)                 # [vL', wL, p0, p1, vR]
        flops += f
        x = ab.permute_legs(bb, x, [1, 2, 3, 4, 0])                   # [wL, p0, p1, vR, vL']
        x, f = self._compose('W1', self.W1, x, 2)                     # [p0', wC, p1, vR, vL']
        flops += f
        x = ab.permute_legs(bb, x, [1, 2, 3, 4, 0])                   # [wC, p1, vR, vL', p0']
        x, f = self._compose('W2', self.W2, x, 2)                     # [p1', wR, vR, vL', p0']
        flops += f
        if self._real_on_complex(theta):
            # the vector stays the B operand: RP^T x instead of x RP, the result legs rotated back as views
            x = ab.permute_legs(bb, x, [1, 2, 3, 4, 0])               # [wR, vR, vL', p0', p1']
            x, f = self._compose('RPt', self._rp_t(), x, 2)           # [vR', vL', p0', p1']
            flops += f
            x = ab.permute_legs(bb, x, [1, 2, 3, 0])                  # [vL', p0', p1', vR']
        else:
            x = ab.permute_legs(bb, x, [3, 4, 0, 2, 1])               # [vL', p0', p1', vR, wR]
            x, f = self._compose('RP', x, self.RP, 2)                 # [vL', p0', p1', vR']
            flops += f
        self.flops_per_matvec = flops
        x.num_codomain = theta.num_codomain
        return x


class TreeChainOperator:
    """A linear map on fusion-tree vectors given as a chain of contractions and leg moves -- what a two-site H_eff on
    fusion-tree tensors is made of (``compose`` and ``permute_legs`` -> ``TreePairMapping::transform_tensor`` in the
    reference).  The symmetry layer stays out: as elsewhere in :mod:`cyten_amd.fusion_tree` its mappings arrive as data.

    `steps`, applied in order to ``X`` on (`codomain`, `domain`):

    * ``('compose_left', A)``: ``X <- A X``, `A` a :class:`fusion_tree.TreeTensor` whose domain is X's codomain;
    * ``('compose_right', B)``: ``X <- X B``, `B` a TreeTensor whose codomain is X's domain;
    * ``('transform', new_codomain, new_domain, codomain_idcs, domain_idcs, mapping)``: one ``ft.transform_tensor``;
    * ``('transform_factorized', new_codomain, new_domain, codomain_idcs, domain_idcs, splitting, fusion)``: one
      ``ft.transform_tensor_factorized`` -- braids and twists inside each side, either map may be None (the identity);
    * ``('partial_compose', B, b_codomain, b_domain, new_codomain, new_domain, insert)``: one ``ft.partial_compose`` of X with
      the blocks `B` (a :class:`fusion_tree.FusionTreeData`) on (`b_codomain`, `b_domain`), `insert` a
      :class:`fusion_tree.TreeInsert` -- a site operator or a gate applied to some legs of one side of X.

    ``matvec`` tracks the spaces through the chain; the constructor checks that every step fits the spaces the one before
    leaves.  ``is_complex``: any operand block, mapping coefficient or insert amplitude is complex.  This is host composition of the existing
    launches (one grouped GEMM per compose, one ``transform_blocks`` per transform, at most two ``tree_strip_many`` per
    factorized transform); recording and replaying the launch
    sequence (:mod:`cyten_amd.replay`) is out of scope here."""

    def __init__(self, bb, steps, codomain, domain):
        self.bb, self.steps, self.codomain, self.domain = bb, [tuple(s) for s in steps], codomain, domain
        cplx = False
        cod, dom = codomain, domain
        for n, st in enumerate(self.steps):
            kind = st[0]
            if kind in ('compose_left', 'compose_right'):
                if len(st) != 2 or not isinstance(st[1], ft.TreeTensor):
                    raise ValueError(f'step {n}: ({kind!r}, TreeTensor) expected')
                op = st[1]
                if kind == 'compose_left':
                    if not ft.same_space(op.domain, cod):
                        raise ValueError(f'step {n}: the domain of A is not the codomain of the vector')
                    cod = op.codomain
                else:
                    if not ft.same_space(op.codomain, dom):
                        raise ValueError(f'step {n}: the codomain of B is not the domain of the vector')
                    dom = op.domain
                cplx = cplx or any(_is_complex_block(b) for b in op.blocks)
            elif kind == 'transform':
                if len(st) != 6:
                    raise ValueError(f'step {n}: (\'transform\', new_codomain, new_domain, codomain_idcs, domain_idcs, mapping) expected')
                cod, dom = st[1], st[2]
                cplx = cplx or any(isinstance(c, (complex, np.complexfloating)) and complex(c).imag != 0.0
                                   for targets in st[5].values() for c in targets.values())
            elif kind == 'transform_factorized':
                if len(st) != 7:
                    raise ValueError(f'step {n}: (\'transform_factorized\', new_codomain, new_domain, codomain_idcs, domain_idcs, splitting, '
                                     'fusion) expected')
                cod, dom = st[1], st[2]
                cplx = cplx or any(isinstance(c, (complex, np.complexfloating)) and complex(c).imag != 0.0
                                   for table in st[5:7] if table is not None for targets in table.values() for c in targets.values())
            elif kind == 'partial_compose':
                if len(st) != 7 or not isinstance(st[1], ft.FusionTreeData) or not isinstance(st[6], ft.TreeInsert):
                    raise ValueError(f'step {n}: (\'partial_compose\', FusionTreeData, b_codomain, b_domain, new_codomain, new_domain, '
                                     'TreeInsert) expected')
                cod, dom = st[4], st[5]
                cplx = cplx or any(_is_complex_block(b) for b in st[1].blocks) or any(
                    complex(amp).imag != 0.0 for lst in st[6].table.values() for _, amp in lst)
            else:
                raise ValueError(f'step {n}: unknown kind {kind!r}')
        self.out_codomain, self.out_domain = cod, dom
        self.is_complex = bool(cplx)

    def matvec(self, x):
        bb = self.bb
        data, cod, dom = x.data, x.codomain, x.domain
        for st in self.steps:
            if st[0] == 'compose_left':
                data, cod = ft.compose(bb, st[1].data, data), st[1].codomain
            elif st[0] == 'compose_right':
                data, dom = ft.compose(bb, data, st[1].data), st[1].domain
            elif st[0] == 'partial_compose':
                _, B, b_cod, b_dom, new_cod, new_dom, insert = st
                data = ft.partial_compose(bb, data, cod, dom, B, b_cod, b_dom, new_cod, new_dom, insert)
                cod, dom = new_cod, new_dom
            elif st[0] == 'transform_factorized':
                _, new_cod, new_dom, codomain_idcs, domain_idcs, splitting, fusion = st
                data = ft.transform_tensor_factorized(bb, data, cod, dom, new_cod, new_dom, codomain_idcs, domain_idcs, splitting, fusion)
                cod, dom = new_cod, new_dom
            else:
                _, new_cod, new_dom, codomain_idcs, domain_idcs, mapping = st
                data = ft.transform_tensor(bb, data, cod, dom, new_cod, new_dom, codomain_idcs, domain_idcs, mapping)
                cod, dom = new_cod, new_dom
        return ft.TreeTensor(data, cod, dom)


class _NotFlat(Exception):
    """The vector left the block structure the flat representation was built for (caught by the solvers' run)."""


class _NeedComplex(_NotFlat):
    """A complex vector met a float64 pool (the operator is complex): the run restarts on complex128 pools."""


def _is_real_scalar(c) -> bool:
    return not isinstance(c, (complex, np.complexfloating)) or complex(c).imag == 0.0


class _TensorOps:
    """Vector operations of the recurrences on block-sparse tensors (one launch per block LIST, per-block host work)."""

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


def tree_pool_layout(codomain, domain, granule=256):
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


class _FlatOps:
    """The same operations on Krylov vectors kept as ONE contiguous pool each: the block offsets of
    the structure are computed once, every ``scale / axpy / inner / norm`` of the recurrences is a single-descriptor
    launch over the whole pool -- no per-block host work, one descriptor copy.  The pools are zero between blocks
    (32-element alignment gaps), so reductions over the flat range are exact.  Only the operator application sees
    tensors: its input is a list of views into the pool, its output is copied back in one batched launch.

    Pools are float64 while the start vector and the operator are real -- the Lanczos / Arnoldi bases of a real operator
    are real whatever the evolution step delta; only the result assembly ``sum_k c_k v_k`` then has complex coefficients,
    ONE launch of the complex linear combination with real sources.  A complex start vector or operator uses complex128
    pools (interleaved, the same offsets).  Every operation dispatches on the dtype of its pools.  HIP backend only;
    anything else uses :class:`_TensorOps`."""

    def __init__(self, bb, H, template, block_inds=None, cplx=False):
        """`template`: a tensor on the legs of the vectors; `block_inds` (default: the template's): the block table of the
        pool -- a superset of the template's when the operator creates blocks the start vector does not have.
        `cplx`: the Krylov vectors are complex128 pools."""
        from .block_backend import _c_strides
        self._bind(bb, H, template, cplx)
        self.block_inds = template.block_inds if block_inds is None else block_inds
        self.shapes = [template.block_shape(r) for r in self.block_inds]
        self.strides = [_c_strides(sh) for sh in self.shapes]
        offs, tot = [], 0
        for sh in self.shapes:
            n = 1
            for x in sh:
                n *= x
            offs.append(tot)
            tot += (n + 31) // 32 * 32
        self.offs, self.total = offs, tot
        self.key = self.block_inds.tobytes()
        self.index = None     # block row -> position, built only if a tensor has fewer blocks than the pool
        # positions of the pool's blocks that any vector so far holds (the start vector's, plus what the operator produced):
        # the pool is laid out over every charge-allowed block, but the operator only ever sees -- and the result only carries --
        # this support, as the reference's tensors do (krylov_based.cpp works on tensors whose block tables grow the same way)
        self.support = set()

    def _bind(self, bb, H, template, cplx):
        from .block_backend import HipBlock
        from . import _lib
        import ctypes
        self.bb, self.H, self.t, self.cplx = bb, H, template, bool(cplx)
        self._HipBlock, self._lib, self._C = HipBlock, _lib, ctypes

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

    def _views(self, buf, which=None):
        bb, mk = self.bb, self._HipBlock._trusted
        idx = range(len(self.offs)) if which is None else which
        return [mk(bb, buf, self.offs[i], self.shapes[i], self.strides[i], True) for i in idx]

    def enter(self, t):
        """tensor -> pool (one memset + one batched copy); a real tensor enters a complex pool as its real plane."""
        if not self.cplx and any(b.is_complex for b in t.blocks):
            raise _NeedComplex()
        buf = self._alloc(True)
        if t.block_inds.tobytes() == self.key:
            which = None
        else:   # fewer blocks than the template (missing blocks are zero); a block outside the template ends flat mode
            if self.index is None:
                self.index = {tuple(r): i for i, r in enumerate(self.block_inds.tolist())}
            try:
                which = [self.index[tuple(r)] for r in t.block_inds.tolist()]
            except KeyError:
                raise _NotFlat()
        views = self._views(buf, which)
        if any(v.shape != tuple(b.shape) for v, b in zip(views, t.blocks)):
            raise _NotFlat()
        self.support.update(range(len(self.offs)) if which is None else which)
        self.bb.copy_many([(v if b.is_complex or not self.cplx else self.bb._plane(v, 0), b) for v, b in zip(views, t.blocks)])
        return buf

    def leave(self, buf):
        t = self.t
        if len(self.support) == len(self.offs):
            return ab.AbelianTensor(t.symmetry, t.legs, self._views(buf), self.block_inds, t.num_codomain, t.labels)
        idx = sorted(self.support)     # (positions ascend with the lexsorted block table)
        return ab.AbelianTensor(t.symmetry, t.legs, self._views(buf, idx), self.block_inds[idx], t.num_codomain, t.labels)

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

    def _gs(self, basis, w, passes, out, off=0):
        bb = self.bb
        fn = bb.lib.cyb_gram_schmidt_c128 if w.is_complex() else bb.lib.cyb_gram_schmidt_f64
        bb.ctx.sync_stream()
        self._lib.check(fn(bb.ctx.handle, self._ptrs(basis), len(basis), self._C.c_void_p(w.data_ptr()), self.total, int(passes),
                           self._C.c_void_p(out.data_ptr() + 8 * off)))

    def _multi(self, kind, basis, w, h, off=0, alpha=1.0):
        bb, C = self.bb, self._C
        cp = w.is_complex()
        bb.ctx.sync_stream()
        hp = C.c_void_p(h.data_ptr() + 8 * off)
        if kind == 'dot':
            fn = bb.lib.cyb_multi_dot_c128 if cp else bb.lib.cyb_multi_dot_f64
            self._lib.check(fn(bb.ctx.handle, self._ptrs(basis), len(basis), C.c_void_p(w.data_ptr()), self.total, hp))
        elif cp:
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
        bb, C, m = self.bb, self._C, len(pools)
        if any(p.is_complex() != self.cplx for p in pools):
            raise _NeedComplex()
        if m == 0 or self.total == 0:
            return np.zeros(0), np.zeros(0, dtype=bool)
        out = bb.ctx.empty(2 * m)
        bb.ctx.sync_stream()
        sfx = 'c128' if self.cplx else 'f64'
        if self._weights_ptr() is None:
            rc = getattr(bb.lib, 'cyb_orthonormalize_' + sfx)(bb.ctx.handle, self._ptrs(pools), m, self.total, float(rcond),
                                                              C.c_void_p(out.data_ptr()))
        else:
            rc = getattr(bb.lib, 'cyb_orthonormalize_weighted_' + sfx)(bb.ctx.handle, self._ptrs(pools), m, self.total, float(rcond),
                                                                       self._weights_ptr(), C.c_void_p(out.data_ptr()))
        self._lib.check(rc)
        r = bb.ctx.d2h(out, 2 * m, np.float64)
        return r[:m].copy(), r[m:] != 0.0

    def _weights_ptr(self):
        """the granule table of the weighted entries (None: the unweighted entries run)"""
        return None

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
        :class:`LanczosEigenpairs`) by ONE cyb_basis_rotate_f64 call IN PLACE: the results replace basis[0 .. k-1] (which are
        returned), basis[k:] is untouched; nothing is downloaded.  The matrix is real, so a complex pool is rotated as its
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

    def combine(self, coeffs, vecs, acc=None):
        """acc + sum_k coeffs[k] vecs[k] in ONE launch over the flat range (the result assembly of the solvers).  Complex
        coefficients or pools: the complex linear combination, float64 pools read as real sources (`src_real`), the
        result a complex pool; `acc` (a complex pool) is updated in place.  Real throughout: the float64 form."""
        bb, L = self.bb, self._lib
        cplx = (any(v.is_complex() for v in vecs) or not all(_is_real_scalar(c) for c in coeffs)
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
        """complex128 copy of a float64 pool."""
        return self.combine([1.0 + 0.0j], [w])

    def lincomb(self, a, w, b, v):
        if w.is_complex() != v.is_complex() or (not w.is_complex() and not (_is_real_scalar(a) and _is_real_scalar(b))):
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
        if w.is_complex():
            a = complex(a)
            self._call('cyb_axpby_batched_c128', self._desc(w, None, out), a.real, a.imag, 0.0, 0.0)
        else:
            self._call('cyb_axpby_batched_f64', self._desc(w, None, out), float(np.real(a)), 0.0)
        return out

    def inner(self, v, w):
        """<v, w> = sum conj(v) w: a float on float64 pools, a complex number otherwise (cyb_dot_batched_c128)."""
        bb = self.bb
        if not v.is_complex() and not w.is_complex():
            res = bb.ctx.empty(1)
            self._call('cyb_dot_batched_f64', self._desc(v, w, None), self._C.c_void_p(res.data_ptr()))
            return float(bb.ctx.d2h(res, 1, np.float64)[0])
        v = v if v.is_complex() else self._promote(v)
        w = w if w.is_complex() else self._promote(w)
        res = bb.ctx.empty(2)
        self._call('cyb_dot_batched_c128', self._desc(v, w, None), self._C.c_void_p(res.data_ptr()))
        re, im = bb.ctx.d2h(res, 2, np.float64)
        return complex(float(re), float(im))

    def norm(self, w):
        if not w.is_complex():
            return float(np.sqrt(self.inner(w, w)))
        # the float64 reduction over the interleaved storage: sum re^2 + im^2
        bb = self.bb
        res = bb.ctx.empty(1)
        self._call('cyb_dot_batched_f64', self._desc(w, w, None, 2 * self.total), self._C.c_void_p(res.data_ptr()))
        return float(np.sqrt(bb.ctx.d2h(res, 1, np.float64)[0]))


class _FlatTreeOps(_FlatOps):
    """:class:`_FlatOps` for fusion-tree vectors.  The pool holds the blocks themselves -- ``leave`` stays a list of views and
    the operator reads and writes plain blocks -- so the inner product sum_c d_c <X_c, Y_c> is not the plain one over the flat
    range: the reductions (``inner``, ``norm``, the fused Gram-Schmidt step, the multi-dot) are the weighted entries of
    krylov_vec.hip, which read the quantum dimension of a granule of 256 elements from a table built ONCE per structure and
    kept on the device (:func:`tree_pool_layout`).  Everything linear (``scale``, ``lincomb``, ``combine``, the multi-axpy) is
    inherited: it does not see the weights."""

    GRANULE = 256

    def __init__(self, bb, H, template, cplx=False):
        from .block_backend import _c_strides
        self._bind(bb, H, template, cplx)
        self.block_inds, self.shapes, self.offs, self.total, self.weights = tree_pool_layout(template.codomain, template.domain,
                                                                                             self.GRANULE)
        self.strides = [_c_strides(sh) for sh in self.shapes]
        self.key = self.block_inds.tobytes()
        self.index = None
        self.support = set()
        self._wdev = bb.ctx.empty(max(len(self.weights), 1))
        if len(self.weights):
            bb.ctx.h2d(self._wdev, self.weights)

    @staticmethod
    def usable(bb, t) -> bool:
        return _FlatOps.usable(bb, t) and tree_pool_layout(t.codomain, t.domain)[3] > 0

    def leave(self, buf):
        idx = None if len(self.support) == len(self.offs) else sorted(self.support)
        rows = self.block_inds if idx is None else self.block_inds[idx]
        return self.t.like(ft.FusionTreeData(rows.copy(), self._views(buf, idx)))

    def _wptr(self):
        return self._C.c_void_p(self._wdev.data_ptr())

    def _weights_ptr(self):
        return self._wptr()

    def _gs(self, basis, w, passes, out, off=0):
        bb = self.bb
        fn = bb.lib.cyb_gram_schmidt_weighted_c128 if w.is_complex() else bb.lib.cyb_gram_schmidt_weighted_f64
        bb.ctx.sync_stream()
        self._lib.check(fn(bb.ctx.handle, self._ptrs(basis), len(basis), self._C.c_void_p(w.data_ptr()), self.total, int(passes),
                           self._wptr(), self._C.c_void_p(out.data_ptr() + 8 * off)))

    def _multi(self, kind, basis, w, h, off=0, alpha=1.0):
        if kind != 'dot':
            return super()._multi(kind, basis, w, h, off, alpha)
        bb, C = self.bb, self._C
        fn = bb.lib.cyb_multi_dot_weighted_c128 if w.is_complex() else bb.lib.cyb_multi_dot_weighted_f64
        bb.ctx.sync_stream()
        self._lib.check(fn(bb.ctx.handle, self._ptrs(basis), len(basis), C.c_void_p(w.data_ptr()), self.total, self._wptr(),
                           C.c_void_p(h.data_ptr() + 8 * off)))

    def inner(self, v, w):
        """<v, w> = sum_c d_c sum conj(v_c) w_c: the weighted multi-dot with the basis [v]"""
        cplx = v.is_complex() or w.is_complex()
        if cplx:
            v = v if v.is_complex() else self._promote(v)
            w = w if w.is_complex() else self._promote(w)
        k = 2 if cplx else 1
        res = self.bb.ctx.empty(k)
        self._multi('dot', [v], w, res)
        r = self.bb.ctx.d2h(res, k, np.float64)
        return complex(float(r[0]), float(r[1])) if cplx else float(r[0])

    def norm(self, w):
        return float(np.sqrt(max(np.real(self.inner(w, w)), 0.0)))


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


class _PoolPart:
    """the blocks of one component of a direct-sum pool: positions first .. first + n - 1 of the pool's block list"""

    def __init__(self, first, block_inds):
        self.first, self.block_inds, self.n = first, block_inds, len(block_inds)
        self.key = block_inds.tobytes()
        self.index = None

    def positions(self, block_inds):
        """pool positions of the blocks of a tensor of this component (_NotFlat: a block the pool does not have)"""
        if block_inds.tobytes() == self.key:
            return list(range(self.first, self.first + self.n))
        if self.index is None:
            self.index = {tuple(r): self.first + i for i, r in enumerate(self.block_inds.tolist())}
        try:
            return [self.index[tuple(r)] for r in block_inds.tolist()]
        except KeyError:
            raise _NotFlat()


class _FlatDirectSumOps(_FlatTreeOps):
    """The pool of a direct sum: the pools of its components -- each with the layout it has alone, abelian
    segments over every charge-allowed block at multiples of 32 elements, tree segments as :func:`tree_pool_layout` -- one
    after the other in ONE allocation, so that every recurrence, the fused CGS2 step and the projected matvec are the single
    launches they are for one tensor.  Without a tree component the unweighted entries run over the whole range; with one,
    every segment starts at a multiple of 256 elements and the weighted entries run with weight 1.0 on the granules of the
    abelian segments.  Gaps are zero.  With ONE component the pool is byte for byte that of :class:`_FlatOps` /
    :class:`_FlatTreeOps`.  ``enter`` is one memset and ONE batched copy over the blocks of all components, ``leave`` a
    direct sum of views; the support is tracked per block, hence per component."""

    def __init__(self, bb, H, template, cplx=False):
        from .block_backend import _c_strides
        self._bind(bb, H, template, cplx)
        self.weighted = any(_is_tree(c) for c in template.components)
        align = self.GRANULE if self.weighted else 32
        self.parts, self.shapes, self.offs, weights, tot = [], [], [], [], 0
        for c in template.components:
            if _is_tree(c):
                inds, shapes, offs, n, w = tree_pool_layout(c.codomain, c.domain, self.GRANULE)
            else:
                inds = ab.AbelianTensor.allowed_block_inds(c.symmetry, c.legs)
                shapes = [c.block_shape(r) for r in inds]
                offs, n = [], 0
                for sh in shapes:
                    k = 1
                    for x in sh:
                        k *= x
                    offs.append(n)
                    n += (k + 31) // 32 * 32
                n = (n + align - 1) // align * align
                w = [1.0] * (n // self.GRANULE) if self.weighted else []
            self.parts.append(_PoolPart(len(self.offs), inds))
            self.offs += [tot + o for o in offs]
            self.shapes += list(shapes)
            weights += list(w)
            tot += n
        self.total = tot
        self.strides = [_c_strides(sh) for sh in self.shapes]
        self.support = set()
        self.weights = np.array(weights, dtype=np.float64)
        if self.weighted:
            self._wdev = bb.ctx.empty(max(len(self.weights), 1))
            if len(self.weights):
                bb.ctx.h2d(self._wdev, self.weights)

    @staticmethod
    def usable(bb, t) -> bool:
        return _FlatOps.usable(bb, t)

    def enter(self, x):
        """direct sum -> pool: one memset + ONE batched copy over the blocks of all components"""
        if not isinstance(x, ds.DirectSum) or len(x) != len(self.parts):
            raise _NotFlat()
        blocks = x.blocks
        if not self.cplx and any(b.is_complex for b in blocks):
            raise _NeedComplex()
        buf = self._alloc(True)
        pos = [p for part, c in zip(self.parts, x.components) for p in part.positions(c.block_inds)]
        views = self._views(buf, pos)
        if any(v.shape != tuple(b.shape) for v, b in zip(views, blocks)):
            raise _NotFlat()
        self.support.update(pos)
        if views:
            self.bb.copy_many([(v if b.is_complex or not self.cplx else self.bb._plane(v, 0), b) for v, b in zip(views, blocks)])
        return buf

    def leave(self, buf):
        comps = []
        for part, t in zip(self.parts, self.t.components):
            idx = [p for p in range(part.first, part.first + part.n) if p in self.support]
            rows = part.block_inds[[p - part.first for p in idx]]
            views = self._views(buf, idx)
            if _is_tree(t):
                comps.append(t.like(ft.FusionTreeData(rows.copy(), views)))
            else:
                comps.append(ab.AbelianTensor(t.symmetry, t.legs, views, rows, t.num_codomain, t.labels))
        return ds.DirectSum(comps)

    def _weights_ptr(self):
        return self._wptr() if self.weighted else None

    def _gs(self, basis, w, passes, out, off=0):
        return (_FlatTreeOps if self.weighted else _FlatOps)._gs(self, basis, w, passes, out, off)

    def _multi(self, kind, basis, w, h, off=0, alpha=1.0):
        return (_FlatTreeOps if self.weighted else _FlatOps)._multi(self, kind, basis, w, h, off, alpha)

    def inner(self, v, w):
        return (_FlatTreeOps if self.weighted else _FlatOps).inner(self, v, w)

    def norm(self, w):
        return (_FlatTreeOps if self.weighted else _FlatOps).norm(self, w)


def _is_tree(t) -> bool:
    return isinstance(t, ft.TreeTensor)


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
    if isinstance(t, ds.DirectSum):
        return _FlatDirectSumOps.usable(bb, t)
    return _FlatTreeOps.usable(bb, t) if _is_tree(t) else _FlatOps.usable(bb, t)


def _mgs(V, basis, w):
    h = []
    for v in basis:
        c = V.inner(v, w)
        h.append(c)
        w = V.lincomb(1.0, w, -c, v)
    return w, np.array(h), V.norm(w)


class LanczosGroundState:
    """Lanczos for the lowest eigenvector of a Hermitian ``H`` (krylov_based.cpp:803-946).

    Options (defaults of krylov_based.cpp:276-288, 808-809): N_min=2, N_max=20, P_tol=1e-14,
    min_gap=1e-12, reortho=False, cutoff=100*eps, E_tol=inf, E_shift=None, N_cache=N_max."""

    def __init__(self, bb, H, psi0, options=None):
        o = dict(options or {})
        self.bb, self.H, self.psi0 = bb, H, psi0
        self.N_min = int(o.get('N_min', 2))
        self.N_max = int(o.get('N_max', 20))
        self.P_tol = float(o.get('P_tol', 1e-14))
        self.min_gap = float(o.get('min_gap', 1e-12))
        self.reortho = bool(o.get('reortho', False))
        self.cutoff = float(o.get('cutoff', np.finfo(np.float64).eps * 100))
        self.E_tol = float(o.get('E_tol', np.inf))
        self.E_shift = o.get('E_shift', None)
        self.N_cache = int(o.get('N_cache', self.N_max))
        self.flat = o.get('flat', True)   # (not a reference option: Krylov vectors as flat pools where possible, _FlatOps)
        self.V = None
        if self.N_min < 2:
            raise ValueError('Should perform at least 2 steps.')
        if self.N_cache < 2:
            raise ValueError('Need to cache at least two vectors.')
        self._psi0_norm = None
        # E_shift shifts the operator INSIDE a projected operator (krylov_based.cpp:289-296): the projection then keeps the
        # ortho vectors at eigenvalue `penalty`, not penalty + E_shift.  (A copy: the caller's operator is not changed.)
        self._shift_outside = self.E_shift is not None
        from .sparse import ProjectedLinearOperator, ShiftedLinearOperator
        if self.E_shift is not None and isinstance(H, ProjectedLinearOperator):
            self.H = H.with_original(ShiftedLinearOperator(H.original_operator, float(self.E_shift), H.bb))
            self._shift_outside = False
        self._reset_krylov_state()

    def _reset_krylov_state(self):
        self._h = np.zeros((self.N_max + 1, self.N_max + 1))
        self.Es = np.zeros((self.N_max, self.N_max))
        self._cache = []
        self._result_krylov = np.ones(1)

    # -- small helpers -------------------------------------------------------------------------
    def _to_cache(self, w):
        self._cache.append(w)
        if len(self._cache) > self.N_cache:
            self._cache.pop(0)

    def _matvec(self, w):
        V = self.V
        out = V.matvec(w)
        if self._shift_outside:
            out = V.lincomb(1.0, out, float(self.E_shift), self._cache[-1])
        return out

    def _solve(self, body):
        """``body()`` with the recurrences on flat pools where the backend allows it (:class:`_FlatOps`): float64 pools
        while the start vector and the operator are real, complex128 pools otherwise (a complex vector out of the operator
        restarts the run on them); a vector that leaves the block structure of psi0 (an operator that creates blocks psi0
        does not have) restarts it on tensors."""
        psi_in = self.psi0
        flat = bool(self.flat) and _flat_usable(self.bb, psi_in)
        cplx = any(_is_complex_block(b) for b in psi_in.blocks) or bool(getattr(self.H, 'is_complex', False))
        modes = ([cplx] if cplx else [False, True]) if flat else []
        modes.append(None)   # tensors
        i = 0
        while True:
            mode = modes[i]
            self.V = _vector_ops(self.bb, self.H, psi_in, mode)
            self._reset_krylov_state()
            try:
                self.psi0 = self.V.enter(psi_in)
                return body()
            except _NeedComplex:
                i += 1
            except _NotFlat:
                i = len(modes) - 1
            finally:
                self.psi0 = psi_in     # (the working copy is a pool buffer: a second run() starts from the caller's tensor again)

    def run(self):
        def body():
            N = self._build_krylov()
            E0 = float(self.Es[N - 1, 0])
            if self.E_shift is not None:
                E0 -= float(self.E_shift)
            if N == 1:
                return E0, self.V.leave(self.psi0), N
            return E0, self.V.leave(self._calc_result_full(N)), N
        return self._solve(body)

    def _build_krylov(self):
        V = self.V
        w = self.psi0
        beta = V.norm(w)
        if beta < self.cutoff:
            raise ValueError(f'Norm of self.psi0 too small: {beta}')
        self.psi0 = V.scale(1.0 / beta, w)
        if self._psi0_norm is None:     # (only LanczosEvolution uses it, krylov_based.cpp:851-854)
            self._psi0_norm = beta
        performed = 0
        for k in range(self.N_max):
            w = V.scale(1.0 / beta, w)
            self._to_cache(w)
            w = self._matvec(w)
            alpha = float(np.real(V.inner(w, self._cache[-1])))   # krylov_based.cpp:861: inner(...).real()
            self._h[k, k] = alpha
            self._calc_result_krylov(k)
            w = V.lincomb(1.0, w, -alpha, self._cache[-1])
            if self.reortho:
                for v in self._cache[:-1]:
                    ov = V.inner(v, w)
                    w = V.lincomb(1.0, w, -ov, v)
            elif k > 0:
                w = V.lincomb(1.0, w, -beta, self._cache[-2])
            beta = V.norm(w)
            self._h[k, k + 1] = self._h[k + 1, k] = beta
            performed = k + 1
            if abs(beta) < self.cutoff or (k + 1 >= self.N_min and self._converged(k)):
                break
        return performed

    def _converged(self, k):
        v0k = self._result_krylov[k]
        ritz_res = abs(v0k) * abs(self._h[k, k + 1])
        gap = max(self.Es[k, 1] - self.Es[k, 0], self.min_gap)
        P_err = (ritz_res / gap) ** 2
        Delta_E0 = self.Es[k - 1, 0] - self.Es[k, 0]
        return P_err < self.P_tol and Delta_E0 < self.E_tol

    def _calc_result_krylov(self, k):
        if k == 0:
            self.Es[0, 0] = self._h[0, 0]
            self._result_krylov = np.ones(1)
            return
        n = k + 1
        E_kr, v_kr = np.linalg.eigh(self._h[:n, :n])
        self.Es[k, :n] = E_kr
        self._result_krylov = v_kr[:, 0].copy()

    def _calc_result_full(self, N):
        V = self.V
        vf = self._result_krylov
        if not (N == len(vf) and len(vf) > 1):
            raise RuntimeError('KrylovBased._calc_result_full: expected N == len(vf) > 1')
        psif = V.scale(float(vf[0]), self.psi0)
        len_cache = len(self._cache)
        for k in range(1, min(len_cache + 1, N)):
            psif = V.lincomb(1.0, psif, float(vf[N - k]), self._cache[len_cache - k])
        self._cache = []
        psif = self._rebuild_krylov_for_result_full(psif, N - len_cache - 1)
        nrm = V.norm(psif)
        return V.scale(1.0 / nrm, psif)

    def _rebuild_krylov_for_result_full(self, psif, n_rebuild):
        """Vectors that fell out of the cache are regenerated from psi0 (krylov_based.cpp:896-920)."""
        V = self.V
        vf = self._result_krylov
        w = self.psi0
        beta = 0.0
        for k in range(max(n_rebuild, 0)):
            self._to_cache(w)
            w = self._matvec(w)
            alpha = self._h[k, k]
            w = V.lincomb(1.0, w, -alpha, self._cache[-1])
            if self.reortho:
                for v in self._cache[:-1]:
                    ov = V.inner(v, w)
                    w = V.lincomb(1.0, w, -ov, v)
            elif k > 0:
                w = V.lincomb(1.0, w, -beta, self._cache[-2])
            beta = self._h[k, k + 1]
            w = V.scale(1.0 / beta, w)
            psif = self._add_to_result(psif, vf[k + 1], w)
        return psif

    def _add_to_result(self, psif, c, w):
        return self.V.lincomb(1.0, psif, float(c), w)


def lanczos(bb, H, psi, options=None):
    """(E0, psi0, N) -- krylov_based.cpp:1022-1025."""
    return LanczosGroundState(bb, H, psi, options).run()


class LanczosEvolution(LanczosGroundState):
    """exp(delta H) psi0 for a Hermitian ``H`` by Lanczos (krylov_based.cpp:948-1019): the Krylov recurrences of
    :class:`LanczosGroundState` (real tridiagonal matrix), the small problem solved as exp(delta E) in the eigenbasis of
    that matrix, converged when the last Krylov coefficient is below P_tol.  With a real ``H`` and a real psi0 the Krylov
    vectors stay float64 whatever delta; the complex coefficients only enter the result assembly."""

    def __init__(self, bb, H, psi0, options=None):
        super().__init__(bb, H, psi0, options)
        self._result_norm = 1.0
        self.delta = None

    def run(self, delta, normalize=None):
        """(psi, N).  `normalize` (default: delta.real == 0): return the normalised state, else the state scaled by
        |psi0| times the norm of the Krylov result, i.e. exp(delta H) psi0 itself."""
        self.delta = delta
        do_normalize = (complex(delta).real == 0.0) if normalize is None else bool(normalize)

        def body():
            V = self.V
            N = self._build_krylov()
            if N == 1:
                res = V.scale(self._result_krylov[0], self.psi0)    # (a phase)
            else:
                res = self._calc_result_full(N)
            if not do_normalize:
                res = V.scale((1.0 if self._psi0_norm is None else self._psi0_norm) * self._result_norm, res)
            return V.leave(res), N
        return self._solve(body)

    def _calc_result_krylov(self, k):
        d = self.delta
        if k == 0:
            e = np.exp(d * self._h[0, 0])
            self._result_norm = float(abs(e))
            self._result_krylov = np.array([e / self._result_norm])
            return
        n = k + 1
        E_kr, v_kr = np.linalg.eigh(self._h[:n, :n])
        r = v_kr @ (np.exp(E_kr * d) * np.conj(v_kr[0]))
        self._result_norm = float(np.linalg.norm(r))
        self._result_krylov = r / self._result_norm

    def _converged(self, k):
        return abs(self._result_krylov[k]) < self.P_tol

    def _calc_result_full(self, N):
        """sum_k c_k v_k as ONE combination of psi0 and the cached vectors (krylov_based.cpp:310-341), the vectors that
        fell out of the cache regenerated and added one at a time."""
        V = self.V
        vf = self._result_krylov
        if not (N == len(vf) and len(vf) > 1):
            raise RuntimeError('KrylovBased._calc_result_full: expected N == len(vf) > 1')
        len_cache = len(self._cache)
        n_loop = min(len_cache + 1, N)
        psif = V.combine([vf[0]] + [vf[N - k] for k in range(1, n_loop)],
                         [self.psi0] + [self._cache[len_cache - k] for k in range(1, n_loop)])
        self._cache = []
        psif = self._rebuild_krylov_for_result_full(psif, N - len_cache - 1)
        nrm = V.norm(psif)
        return V.scale(1.0 / nrm, psif)

    def _add_to_result(self, psif, c, w):
        return self.V.combine([c], [w], acc=psif)


def argsort_which(values, which):
    """Order of Ritz values by the reference's `which` names and aliases (krylov_based.cpp:166-195)."""
    v = np.asarray(values, dtype=np.complex128)
    if which in ('LM', 'm>'):
        key = -np.abs(v)
    elif which in ('SM', 'm<'):
        key = np.abs(v)
    elif which in ('LR', '>', 'LA'):
        key = -v.real
    elif which in ('SR', '<', 'SA'):
        key = v.real
    elif which == 'LI':
        key = -v.imag
    elif which == 'SI':
        key = v.imag
    else:
        key = v.real
    return np.argsort(key, kind='stable')


class Arnoldi(LanczosGroundState):
    """Arnoldi for eigenvalues of a general (non-Hermitian) ``H`` (krylov_based.cpp:532-695): complex Hessenberg matrix,
    modified Gram-Schmidt against every cached vector in the reference's order, Ritz pairs from numpy.linalg.eig sorted
    by `which`.  Options beyond LanczosGroundState's: which='LM', num_ev=1, E_tol=inf; requires N_cache >= N_max."""

    def __init__(self, bb, H, psi0, options=None):
        o = dict(options or {})
        super().__init__(bb, H, psi0, o)
        self.which = str(o.get('which', 'LM'))
        self.num_ev = int(o.get('num_ev', 1))

    def _reset_krylov_state(self):
        self._h = np.zeros((self.N_max + 1, self.N_max + 1), dtype=np.complex128)
        self.Es = np.zeros((self.N_max, self.N_max), dtype=np.complex128)
        self._cache = []
        self._result_krylov = np.ones((1, 1), dtype=np.complex128)

    def _to_cache(self, w):
        self._cache.append(w)
        if len(self._cache) > self.N_cache:
            raise RuntimeError('Arnoldi cache exceeded N_cache')

    def run(self):
        """(Es, psis, N): the first num_ev Ritz values in `which` order and their normalised Ritz vectors."""
        if self.N_cache < self.N_max:
            raise ValueError('Arnoldi requires N_cache >= N_max')

        def body():
            N = self._build_krylov()
            E0 = [complex(self.Es[N - 1, i]) for i in range(self.num_ev)]
            if self.E_shift is not None:
                E0 = [e - self.E_shift for e in E0]
            if N == 1:
                return E0, [self.V.leave(self.psi0)], N
            return E0, [self.V.leave(p) for p in self._calc_result_full_multi(N)], N
        return self._solve(body)

    def _build_krylov(self):
        V = self.V
        w = self.psi0
        w_norm = V.norm(w)
        self.psi0 = V.scale(1.0 / w_norm, w)
        performed = 0
        for k in range(self.N_max):
            w = V.scale(1.0 / w_norm, w)
            self._to_cache(w)
            w = self._matvec(w)
            for i, v in enumerate(self._cache):
                ov = V.inner(v, w)
                self._h[i, k] = ov
                w = V.lincomb(1.0, w, -ov, v)
            w_norm = V.norm(w)
            self._h[k + 1, k] = w_norm
            self._calc_result_krylov(k)
            performed = k + 1
            if w_norm < self.cutoff or (k + 1 >= self.N_min and self._converged(k)):
                break
        return performed

    def _calc_result_krylov(self, k):
        if k == 0:
            self.Es[0, 0] = self._h[0, 0]
            self._result_krylov = np.ones((1, 1), dtype=np.complex128)
            return
        n = k + 1
        E_kr, v_kr = np.linalg.eig(self._h[:n, :n])
        order = argsort_which(E_kr, self.which)
        self.Es[k, :n] = E_kr[order]
        self._result_krylov = v_kr[:, order]

    def _converged(self, k):
        v0k = self._result_krylov[k, 0]
        ritz_res = abs(v0k) * abs(self._h[k + 1, k])
        min_diff = np.inf
        for i in range(self.num_ev):
            d = np.abs(self.Es[k, i + 1:self.N_max] - self.Es[k, i])
            min_diff = min(min_diff, float(d.min()) if len(d) else np.inf)
        gap = max(min_diff, self.min_gap)
        P_err = (ritz_res / gap) ** 2
        Delta_E0 = self.Es[k - 1, 0] - self.Es[k, 0]
        return P_err < self.P_tol and Delta_E0.real < self.E_tol

    def _calc_result_full_multi(self, N):
        V = self.V
        if len(self._cache) < N:
            raise RuntimeError('Arnoldi._calc_result_full: Krylov basis shorter than N')
        psis = []
        for i in range(min(N, self.num_ev)):
            # real_if_close: the dominant eigenvector of a real operator stays real (the power-method answer)
            vf = np.real_if_close(self._result_krylov[:N, i])
            psi = V.combine(list(vf), self._cache[:N])
            psis.append(V.scale(1.0 / V.norm(psi), psi))
        return psis


class ArnoldiEvolution(Arnoldi):
    """exp(delta H) psi0 for a general ``H`` by Arnoldi (krylov_based.cpp:697-800): the small problem solved through
    numpy.linalg.eig and a linear solve for the start vector's coefficients; converged when the last Krylov coefficient is
    below P_tol.  `normalize` defaults to False."""

    def __init__(self, bb, H, psi0, options=None):
        super().__init__(bb, H, psi0, options)
        self._result_norm = 1.0
        self.delta = None
        # (Arnoldi._build_krylov does not record it)
        self._psi0_norm = _vector_ops(bb, H, psi0, None).norm(psi0)

    def run(self, delta, normalize=None):
        if self.N_cache < self.N_max:
            raise ValueError('ArnoldiEvolution requires N_cache >= N_max')
        self.delta = delta
        do_normalize = False if normalize is None else bool(normalize)

        def body():
            V = self.V
            N = self._build_krylov()
            res = V.scale(self._result_krylov[0], self.psi0) if N == 1 else self._calc_result_full_evolution(N)
            if not do_normalize:
                res = V.scale(self._psi0_norm * self._result_norm, res)
            return V.leave(res), N
        return self._solve(body)

    def _calc_result_krylov(self, k):
        d = self.delta
        if k == 0:
            e = np.exp(d * self._h[0, 0])
            self._result_norm = float(abs(e))
            self._result_krylov = np.array([e / self._result_norm])
            return
        n = k + 1
        E_kr, v_kr = np.linalg.eig(self._h[:n, :n])
        e0 = np.zeros(n, dtype=np.complex128)
        e0[0] = 1.0
        coeff = np.linalg.solve(v_kr, e0)
        r = v_kr @ (np.exp(E_kr * d) * coeff)
        self._result_norm = float(np.linalg.norm(r))
        self._result_krylov = r / self._result_norm

    def _converged(self, k):
        return abs(self._result_krylov[k]) < self.P_tol

    def _calc_result_full_evolution(self, N):
        V = self.V
        if len(self._cache) < N:
            raise RuntimeError('ArnoldiEvolution: Krylov basis shorter than N')
        psif = V.combine(list(self._result_krylov[:N]), self._cache[:N])
        return V.scale(1.0 / V.norm(psif), psif)


_WHICH_NAMES = ('LM', 'm>', 'SM', 'm<', 'LR', '>', 'LA', 'SR', '<', 'SA', 'LI', 'SI')


class LanczosEigenpairs(LanczosGroundState):
    """Several eigenpairs of a Hermitian ``H`` by thick-restart Lanczos (Wu & Simon, SIAM J. Matrix Anal. Appl. 22 (2000)) --
    what the reference offers as ``HermitianNumpyArrayLinearOperator.eigenvectors`` / ``lanczos_arpack`` through a flat host
    array per matvec (sparse.py:410-504), here on the vectors of the other solvers: pools where the backend allows it.

    One bounded basis of `N_max` = m vectors.  A step is ``w = H v_j``, the fused CGS2 call against ALL of v_0 .. v_j (full
    reorthogonalisation: one library call and one download per step) and ``v_{j+1} = w / beta``; the projection T of H is real
    symmetric: tridiagonal, after a restart an arrow (diagonal + one row) followed by a tridiagonal.  Only T[j, j] = Re h_j and
    the new beta are taken from the step; the other coefficients are rounding (below the arrow) or repeat the couplings the
    restart predicted (on its row): ``coupling_error`` keeps the largest difference seen.  With j == m the basis is rotated onto
    the `keep` = l Ritz vectors first in `which` order (``V.rotate``: on pools ONE in-place kernel call), v_m becomes v_l
    and the couplings are beta S[m-1, i].  Ritz pair i has the residual estimate |beta S[j-1, i]|; the run ends when the first
    `num_ev` are <= tol max(|theta_i|, tiny), or when beta < cutoff max|T|: the basis then spans an invariant subspace, its
    min(num_ev, j) pairs are exact and are returned -- FEWER than num_ev pairs is a documented outcome of a start vector that
    lives in a small invariant subspace, not an error.

    As with ARPACK, one start vector finds ONE copy of a degenerate eigenvalue: the Krylov space of a single vector holds one
    vector of every eigenspace.  (Rounding eventually brings further copies in, late and unreliably; a block method is the
    tool for degenerate levels.)

    Options: num_ev=1, which='SA' (any name of :func:`argsort_which`), N_max=max(2 num_ev + 1, 20) (> num_ev),
    keep=num_ev + (N_max - num_ev) // 2 clipped to [num_ev, N_max - 1], tol=1e-10 (0.0: machine eps), max_restarts=100
    (RuntimeError with the residual estimates when exceeded), cutoff=100 eps, flat=True (N_max <= 64, else tensors), E_shift
    as in :class:`LanczosGroundState`.  After ``run``: ``restarts``, ``matvecs``, ``residuals``, ``coupling_error``, ``T``."""

    def __init__(self, bb, H, psi0, options=None):
        o = dict(options or {})
        self.num_ev = int(o.get('num_ev', 1))
        self.which = o.get('which', 'SA')
        if self.num_ev < 1:
            raise ValueError('num_ev must be at least 1')
        if self.which not in _WHICH_NAMES:
            raise ValueError(f'unknown which: {self.which!r}')
        m = int(o.get('N_max', max(2 * self.num_ev + 1, 20)))
        if not self.num_ev < m:
            raise ValueError(f'num_ev = {self.num_ev} pairs need a basis of N_max > num_ev vectors, got {m}')
        default_keep = min(max(self.num_ev + (m - self.num_ev) // 2, self.num_ev), m - 1)
        self.keep = int(o.get('keep', default_keep))
        if not self.num_ev <= self.keep <= m - 1:
            raise ValueError(f'keep = {self.keep} outside [num_ev, N_max - 1] = [{self.num_ev}, {m - 1}]')
        tol = float(o.get('tol', 1e-10))
        self.tol = tol if tol > 0.0 else float(np.finfo(np.float64).eps)
        self.max_restarts = int(o.get('max_restarts', 100))
        base = {k: o[k] for k in ('cutoff', 'flat', 'E_shift') if k in o}
        super().__init__(bb, H, psi0, dict(base, N_max=m))
        if m > _FlatOps.MAX_BASIS:      # (the fused step and the rotation take at most that many vectors)
            self.flat = False
        self.restarts = self.matvecs = 0
        self.residuals = np.zeros(0)
        self.coupling_error = 0.0
        self.T = np.zeros((m + 1, m + 1))

    def _orthogonalize(self, basis, w):
        V = self.V
        w, h, beta = V.project_out(basis, w, passes=2)
        if not isinstance(V, _FlatOps):
            # the tensor operations run ONE pass of modified Gram-Schmidt: a second one, as the fused CGS2 step has
            w, h2, beta = V.project_out(basis, w, passes=2)
            h = np.asarray(h) + np.asarray(h2)
        return w, np.asarray(h), float(beta)

    def run(self):
        """(Es, vectors, N): the Ritz values in `which` order (an ndarray of min(num_ev, dimension of the Krylov space)
        floats), their orthonormal Ritz vectors and the number of matvecs."""
        return self._solve(self._run)

    def _run(self):
        V, m, nev, l = self.V, self.N_max, self.num_ev, self.keep
        tiny = float(np.finfo(np.float64).tiny)
        beta = V.norm(self.psi0)
        if beta < self.cutoff:
            raise ValueError(f'Norm of self.psi0 too small: {beta}')
        basis = [V.scale(1.0 / beta, self.psi0)]
        T = self.T = np.zeros((m + 1, m + 1))
        self.restarts = self.matvecs = 0
        self.coupling_error = 0.0
        j = 0
        while True:
            self._cache = [basis[j]]          # (_matvec adds E_shift times the vector it finds there)
            w = self._matvec(basis[j])
            self.matvecs += 1
            w, h, beta = self._orthogonalize(basis[:j + 1], w)
            T[j, j] = float(np.real(h[j]))
            if j > 0:
                self.coupling_error = max(self.coupling_error, float(np.abs(h[:j] - T[:j, j]).max()))
            T[j + 1, j] = T[j, j + 1] = beta
            j += 1
            broke = beta == 0.0 or beta < self.cutoff * float(np.abs(T[:j + 1, :j + 1]).max())
            if not broke and j < nev:
                basis.append(V.scale(1.0 / beta, w))
                continue
            theta, S = np.linalg.eigh(T[:j, :j])
            order = argsort_which(theta, self.which)
            theta, S = theta[order], S[:, order]
            n_out = min(nev, j)
            self.residuals = np.abs(beta * S[j - 1, :n_out])
            if broke or bool(np.all(self.residuals <= self.tol * np.maximum(np.abs(theta[:n_out]), tiny))):
                break
            basis.append(V.scale(1.0 / beta, w))
            if j == m:
                if self.restarts >= self.max_restarts:
                    raise RuntimeError(f'LanczosEigenpairs: not converged after {self.restarts} restarts and {self.matvecs} '
                                       f'matvecs; residual estimates {self.residuals.tolist()}')
                basis = list(V.rotate(basis[:m], S[:, :l])) + [basis[m]]
                T[:] = 0.0
                T[np.arange(l), np.arange(l)] = theta[:l]
                T[l, :l] = T[:l, l] = beta * S[m - 1, :l]
                j = l
                self.restarts += 1
        vecs = V.rotate(basis[:j], S[:, :n_out])
        self._cache = []
        Es = theta[:n_out].copy()
        if self.E_shift is not None:
            Es -= float(self.E_shift)
        return Es, [V.leave(y) for y in vecs], self.matvecs


def eigenvectors(bb, H, psi0, num_ev=1, which='SA', **options):
    """(eta, vectors) -- the return of the reference's ``HermitianNumpyArrayLinearOperator.eigenvectors`` (sparse.py:502-504):
    `num_ev` eigenvalues of the Hermitian ``H`` in `which` order as an ndarray and the list of their eigenvectors, found from
    the start vector `psi0` by :class:`LanczosEigenpairs` (whose options are the keywords)."""
    Es, vecs, _ = LanczosEigenpairs(bb, H, psi0, dict(options, num_ev=num_ev, which=which)).run()
    return Es, vecs


def compatible(a, b) -> bool:
    """two vectors a solver can combine: direct sums of one length with compatible components, fusion-tree tensors on the
    same spaces, abelian tensors on the same legs -- never a tensor and a direct sum"""
    if isinstance(a, ds.DirectSum) or isinstance(b, ds.DirectSum):
        return ds.compatible(a, b)
    return _same_legs(a, b)


def _same_legs(a, b) -> bool:
    if _is_tree(a) or _is_tree(b):
        return (_is_tree(a) and _is_tree(b) and ft.same_space(a.codomain, b.codomain) and ft.same_space(a.domain, b.domain))
    return len(a.legs) == len(b.legs) and all(
        x.sign == y.sign and np.array_equal(x.sectors, y.sectors) and np.array_equal(x.mults, y.mults)
        for x, y in zip(a.legs, b.legs))


class GMRES:
    """Restarted GMRES for ``A x = b`` (krylov_based.cpp:358-530): Arnoldi with Givens rotations, a back-substitution per
    cycle and a restart from the current x.  Options and defaults of :369-373: N_min=5, N_max=20, restart=10, res=1e-8 (no
    N_min >= 2 check); ``flat`` (not a reference option) as in the other solvers.

    Vectors are flat pools where the backend allows it: float64 while A, x and b are real, complex128 otherwise (a complex
    shift or a complex b); the Arnoldi step orthogonalises by ONE fused CGS2 call (_FlatOps.project_out), the reference's
    modified Gram-Schmidt on tensors.  x += sum_i y_i q_i is one combine.

    Two deliberate deviations from the reference:

    1. Unitary Givens rotations.  The reference takes t = sqrt(v1^2 + v2^2), c = v1 / t, s = v2 / t and rotates with
       [[c, s], [-s, c]] (:471-498), which is not unitary for complex entries: |e1[k+1]| is then not the residual, y does
       not minimise it, and v1^2 + v2^2 = 0 divides by zero.  Here t = sqrt(|v1|^2 + |v2|^2) and H and e1 are rotated
       with [[conj(c), conj(s)], [-s, c]]: the reference's formula for real data, unitary for complex data, so |e1[k+1]| /
       |b| is the true relative residual of the cycle.
    2. Exact breakdown.  A new Krylov vector of norm 0 ends the cycle as converged (the reference would go on and divide by
       zero before N_min)."""

    def __init__(self, bb, A, x, b, options=None):
        o = dict(options or {})
        if A is None:
            raise ValueError('A must not be null')
        if x is None or b is None:
            raise ValueError('x and b must not be null')
        if not compatible(x, b):
            raise ValueError('x and b must have the same legs')
        self.bb, self.A, self.x_in, self.b_in = bb, A, x, b
        self.options = o
        self.N_min = int(o.get('N_min', 5))
        self.N_max = int(o.get('N_max', 20))
        self.restart = int(o.get('restart', 10))
        self.res = float(o.get('res', 1e-8))
        self.flat = o.get('flat', True)
        flat = bool(self.flat) and _flat_usable(bb, b)
        cplx = (any(_is_complex_block(t) for v in (x, b) for t in v.blocks) or bool(getattr(A, 'is_complex', False)))
        self._modes = ([cplx] if cplx else [False, True]) if flat else []
        self._modes.append(None)   # tensors
        self._mode_i = 0
        self._start_any()

    # -- state -------------------------------------------------------------------------------------
    def _start_any(self):
        """The constructor's work (:375-386) in the first vector representation that holds: pools, else tensors."""
        while True:
            try:
                self._start(self._modes[self._mode_i])
                return
            except _NeedComplex:
                self._mode_i += 1
            except _NotFlat:
                self._mode_i = len(self._modes) - 1

    def _start(self, mode):
        bb = self.bb
        self.V = _vector_ops(bb, self.A, self.b_in, mode)
        V = self.V
        self.x = V.enter(self.x_in)
        self.b = V.enter(self.b_in)
        r0 = V.lincomb(1.0, self.b, -1.0, V.matvec(self.x))
        self.rs = [r0]
        self.b_norm = V.norm(self.b)
        self.r_norm = V.norm(r0)
        self.total_error = [[self.r_norm / self._denom()]]
        self.total_iters = []
        self.qs = [V.scale(1.0 / self.r_norm, r0) if self.r_norm > 0 else r0]
        self._init_hessenberg()

    def _denom(self):
        return self.b_norm if self.b_norm != 0.0 else 1.0

    def _init_hessenberg(self):
        self.sine = np.zeros(self.N_max, dtype=np.complex128)
        self.cosine = np.zeros(self.N_max, dtype=np.complex128)
        self.e1 = np.zeros(self.N_max + 1, dtype=np.complex128)
        self.e1[0] = self.r_norm
        self.H = np.zeros((self.N_max + 1, self.N_max), dtype=np.complex128)
        self.y = np.zeros(0, dtype=np.complex128)
        self._h_next = None

    def H_numpy(self):
        """The (N_max + 1) x N_max Hessenberg matrix (complex128), rotated to upper triangular as far as the cycle got."""
        return self.H.copy()

    # -- the iteration -----------------------------------------------------------------------------
    def run(self):
        """(x, rel_residual, total_error, total_iters): total_error holds one list per cycle (the residual after the restart,
        then one entry per step), total_iters the steps of each cycle, rel_residual = |A x - b| / |b| recomputed at the end."""
        while True:
            try:
                return self._run()
            except _NeedComplex:
                self._mode_i += 1
            except _NotFlat:
                self._mode_i = len(self._modes) - 1
            self._start_any()

    def _run(self):
        V = self.V
        if self.total_error[0][0] < self.res:
            return V.leave(self.x), self.total_error[0][0], self.total_error, self.total_iters
        for _ in range(self.restart):
            converged = False
            performed = 0
            for k in range(self.N_max):
                self.arnoldi(k)
                self.apply_givens_rotation(k)
                self.e1[k + 1] = -self.sine[k] * self.e1[k]
                self.e1[k] = np.conj(self.cosine[k]) * self.e1[k]
                # the residual is the last element of the rotated right-hand side
                error = float(abs(self.e1[k + 1])) / self._denom()
                self.total_error[-1].append(error)
                performed = k + 1
                if (error < self.res and k >= self.N_min) or self._h_next == 0.0:
                    converged = True
                    break
            self.total_iters.append(performed)
            self.backsolve(performed)
            y = [_plain_scalar(c) for c in self.y[:performed]]
            self.x = V.combine(y, self.qs[:performed], acc=self.x)
            if not converged:
                self.reset()
            else:
                break
        rel = V.norm(V.lincomb(1.0, V.matvec(self.x), -1.0, self.b))
        if self.b_norm != 0.0:
            rel /= self.b_norm
        return V.leave(self.x), rel, self.total_error, self.total_iters

    def arnoldi(self, k):
        """q = A q_k, orthogonalised against q_0..q_k (:453-469): column k of H and |q| (fused CGS2 on pools)."""
        V = self.V
        q = V.matvec(self.qs[-1])
        q, h, h_next = V.project_out(self.qs[:k + 1], q, 2)
        self.H[:k + 1, k] = h
        self.H[k + 1, k] = h_next
        if h_next > 0:
            q = V.scale(1.0 / h_next, q)
        self.qs.append(q)
        self._h_next = h_next

    def apply_givens_rotation(self, k):
        """Rotate column k by the earlier rotations, then eliminate H[k+1, k] (:471-487; unitary form, see the class)."""
        H, c, s = self.H, self.cosine, self.sine
        for i in range(k):
            temp = np.conj(c[i]) * H[i, k] + np.conj(s[i]) * H[i + 1, k]
            H[i + 1, k] = -s[i] * H[i, k] + c[i] * H[i + 1, k]
            H[i, k] = temp
        self.givens_rotation(k)
        H[k, k] = np.conj(c[k]) * H[k, k] + np.conj(s[k]) * H[k + 1, k]
        H[k + 1, k] = 0

    def givens_rotation(self, k):
        """c, s with [[conj(c), conj(s)], [-s, c]] (v1, v2) = (t, 0) (:489-498 with |v|^2 in place of v^2)."""
        v1, v2 = self.H[k, k], self.H[k + 1, k]
        t = np.sqrt(v1.real * v1.real + v1.imag * v1.imag + v2.real * v2.real + v2.imag * v2.imag)
        if t == 0.0:   # (a zero column: nothing to eliminate)
            self.cosine[k], self.sine[k] = 1.0, 0.0
            return
        self.cosine[k] = v1 / t
        self.sine[k] = v2 / t

    def backsolve(self, k):
        """y = R^-1 e1 over the first k rows (:500-513)."""
        y = np.zeros(k, dtype=np.complex128)
        for i in range(k - 1, -1, -1):
            y[i] = self.e1[i]
            for j in range(i + 1, k):
                y[i] -= self.H[i, j] * y[j]
            y[i] /= self.H[i, i]
        self.y = y

    def reset(self):
        """Restart from the current x (:515-530)."""
        V = self.V
        r = V.lincomb(1.0, self.b, -1.0, V.matvec(self.x))
        self.rs.append(r)
        self.r_norm = V.norm(r)
        self.total_error.append([self.r_norm / self._denom()])
        self.qs = [V.scale(1.0 / self.r_norm, r) if self.r_norm > 0 else r]
        self._init_hessenberg()


def _plain_scalar(c):
    """A complex coefficient with a zero imaginary part as a float: float64 pools stay real."""
    c = complex(c)
    return c.real if c.imag == 0.0 else c
