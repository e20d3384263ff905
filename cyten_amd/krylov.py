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
* Every solver takes fusion-tree vectors (:class:`cyten_amd.fusion_tree.TreeTensor`) as well, and direct sums of both kinds
  (:class:`cyten_amd.direct_sum.DirectSum`): the recurrences are the same code, the vector operations come from
  :mod:`cyten_amd.krylov_vectors` -- on tensors, or on pools whose layout holds the components one after the other and whose
  reductions carry the quantum dimension of the coupled sector where there is a tree;
  :class:`TreeChainOperator` is an operator to apply to fusion-tree vectors.

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
# the vectors of the solvers live in krylov_vectors; the names below are reached through this module as well (the solvers look
# `_vector_ops` and `_flat_usable` up HERE, so that replacing them on this module redirects a run)
from .krylov_vectors import (PoolLayout, _DirectSumOps, _FlatDirectSumOps, _FlatOps, _FlatTreeOps, _NeedComplex,  # noqa: F401
                             _NotFlat, _TensorOps, _TreeTensorOps, _flat_usable, _vector_ops, tree_pool_layout)


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


class _Fallback:
    """The representations of the Krylov vectors a run tries, in order: flat pools where the backend allows it
    (:class:`_FlatOps`) -- float64 pools while the vectors and the operator are real (`cplx` False), then complex128 pools --
    and tensors last.  ``run(attempt)`` calls ``attempt(mode)`` (`mode` as :func:`_vector_ops` takes it) until one returns: a
    complex vector out of the operator (_NeedComplex) moves on to the next representation, a vector that leaves the block
    structure of the template (_NotFlat: an operator that creates blocks the pool does not have) to tensors.  The position is
    kept, so an object that is kept goes on where it stands."""

    def __init__(self, bb, flat, template, cplx):
        flat = bool(flat) and _flat_usable(bb, template)
        self.modes = (([cplx] if cplx else [False, True]) if flat else []) + [None]
        self.i = 0

    def run(self, attempt):
        while True:
            try:
                return attempt(self.modes[self.i])
            except _NeedComplex:
                self.i += 1
            except _NotFlat:
                self.i = len(self.modes) - 1


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
        """``body()`` in the first representation of the vectors that holds (:class:`_Fallback`), every ``run`` from the first
        one again."""
        psi_in = self.psi0
        cplx = any(_is_complex_block(b) for b in psi_in.blocks) or bool(getattr(self.H, 'is_complex', False))

        def attempt(mode):
            self.V = _vector_ops(self.bb, self.H, psi_in, mode)
            self._reset_krylov_state()
            try:
                self.psi0 = self.V.enter(psi_in)
                return body()
            finally:
                self.psi0 = psi_in     # (the working copy is a pool buffer: a second run() starts from the caller's tensor again)
        return _Fallback(self.bb, self.flat, psi_in, cplx).run(attempt)

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
            w, alpha = self._lanczos_step(k, V.scale(1.0 / beta, w), beta)
            self._h[k, k] = alpha
            self._calc_result_krylov(k)
            beta = V.norm(w)
            self._h[k, k + 1] = self._h[k + 1, k] = beta
            performed = k + 1
            if abs(beta) < self.cutoff or (k + 1 >= self.N_min and self._converged(k)):
                break
        return performed

    def _lanczos_step(self, k, v, beta, alpha=None):
        """Step k of the three-term recurrence on the normalised v = v_k, which goes to the cache: (H v_k - alpha v_k - beta
        v_{k-1}, alpha), with full reorthogonalisation against the cache in place of the beta term if `reortho`.  `alpha`
        None: taken as Re <H v_k, v_k>; given (the rebuild of vectors that fell out of the cache): the recorded one."""
        V = self.V
        self._to_cache(v)
        w = self._matvec(v)
        if alpha is None:
            alpha = float(np.real(V.inner(w, self._cache[-1])))   # krylov_based.cpp:861: inner(...).real()
        w = V.lincomb(1.0, w, -alpha, self._cache[-1])
        if self.reortho:
            for u in self._cache[:-1]:
                ov = V.inner(u, w)
                w = V.lincomb(1.0, w, -ov, u)
        elif k > 0:
            w = V.lincomb(1.0, w, -beta, self._cache[-2])
        return w, alpha

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
            w, _ = self._lanczos_step(k, w, beta, self._h[k, k])
            beta = self._h[k, k + 1]
            w = V.scale(1.0 / beta, w)
            psif = self._add_to_result(psif, vf[k + 1], w)
        return psif

    def _add_to_result(self, psif, c, w):
        return self.V.lincomb(1.0, psif, float(c), w)


def lanczos(bb, H, psi, options=None):
    """(E0, psi0, N) -- krylov_based.cpp:1022-1025."""
    return LanczosGroundState(bb, H, psi, options).run()


class _Evolution:
    """What the two evolution solvers share, mixed in before the eigensolver whose ``_build_krylov`` they run: ``run``, the
    coefficients of exp(delta H) psi0 in the Krylov basis from the small matrix, normalised, and the convergence test on the
    last of them.  A solver says how exp(delta h) e_0 is taken (``_small_exp``), how the result is assembled (``_evolved``) and
    what `normalize` defaults to (``_normalize_default``)."""

    def __init__(self, bb, H, psi0, options=None):
        super().__init__(bb, H, psi0, options)
        self._result_norm = 1.0
        self.delta = None

    def _check_run(self):
        pass

    def run(self, delta, normalize=None):
        """(psi, N).  `normalize` None: the solver's default; True: return the normalised state, else the state scaled by
        |psi0| times the norm of the Krylov result, i.e. exp(delta H) psi0 itself."""
        self._check_run()
        self.delta = delta
        do_normalize = self._normalize_default(delta) if normalize is None else bool(normalize)

        def body():
            V = self.V
            N = self._build_krylov()
            res = V.scale(self._result_krylov[0], self.psi0) if N == 1 else self._evolved(N)    # (N == 1: a phase)
            if not do_normalize:
                res = V.scale(self._psi0_norm * self._result_norm, res)
            return V.leave(res), N
        return self._solve(body)

    def _calc_result_krylov(self, k):
        if k == 0:
            e = np.exp(self.delta * self._h[0, 0])
            self._result_norm = float(abs(e))
            self._result_krylov = np.array([e / self._result_norm])
            return
        r = self._small_exp(self._h[:k + 1, :k + 1], self.delta)
        self._result_norm = float(np.linalg.norm(r))
        self._result_krylov = r / self._result_norm

    def _converged(self, k):
        return abs(self._result_krylov[k]) < self.P_tol


class LanczosEvolution(_Evolution, LanczosGroundState):
    """exp(delta H) psi0 for a Hermitian ``H`` by Lanczos (krylov_based.cpp:948-1019): the Krylov recurrences of
    :class:`LanczosGroundState` (real tridiagonal matrix), the small problem solved as exp(delta E) in the eigenbasis of
    that matrix, converged when the last Krylov coefficient is below P_tol.  With a real ``H`` and a real psi0 the Krylov
    vectors stay float64 whatever delta; the complex coefficients only enter the result assembly.  `normalize` defaults to
    delta.real == 0."""

    @staticmethod
    def _normalize_default(delta):
        return complex(delta).real == 0.0

    @staticmethod
    def _small_exp(h, d):
        E_kr, v_kr = np.linalg.eigh(h)
        return v_kr @ (np.exp(E_kr * d) * np.conj(v_kr[0]))

    def _evolved(self, N):
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


class ArnoldiEvolution(_Evolution, Arnoldi):
    """exp(delta H) psi0 for a general ``H`` by Arnoldi (krylov_based.cpp:697-800): the small problem solved through
    numpy.linalg.eig and a linear solve for the start vector's coefficients; converged when the last Krylov coefficient is
    below P_tol.  `normalize` defaults to False."""

    def __init__(self, bb, H, psi0, options=None):
        super().__init__(bb, H, psi0, options)
        self._psi0_norm = ds.vector_norm(bb, psi0)      # (Arnoldi._build_krylov does not record it)

    def _check_run(self):
        if self.N_cache < self.N_max:
            raise ValueError('ArnoldiEvolution requires N_cache >= N_max')

    @staticmethod
    def _normalize_default(delta):
        return False

    @staticmethod
    def _small_exp(h, d):
        E_kr, v_kr = np.linalg.eig(h)
        e0 = np.zeros(len(h), dtype=np.complex128)
        e0[0] = 1.0
        return v_kr @ (np.exp(E_kr * d) * np.linalg.solve(v_kr, e0))

    def _evolved(self, N):
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
        if not V.fused_cgs2:
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


compatible = ds.vectors_compatible     # (GMRES compares x and b with it)


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
        cplx = (any(_is_complex_block(t) for v in (x, b) for t in v.blocks) or bool(getattr(A, 'is_complex', False)))
        # kept across run() calls: a second run goes on in the representation the first one ended in
        self._fallback = _Fallback(bb, self.flat, b, cplx)
        self._fallback.run(self._start)

    # -- state -------------------------------------------------------------------------------------
    def _start(self, mode):
        """The constructor's work (:375-386) with the vectors in the representation `mode`."""
        bb = self.bb
        self._mode = mode
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
        def attempt(mode):
            if mode is not self._mode:      # (the representation the state is in did not hold: start again in the next one)
                self._start(mode)
            return self._run()
        return self._fallback.run(attempt)

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
