"""Inputs of the Krylov solvers on fusion-tree vectors shared by tests/test_tree_krylov.py (numpy stand-in: the host logic
without a device) and tests/test_gpu_tree_krylov.py (HipBlockBackend: the same inputs, the same criteria).

The structure: four coupled sectors with quantum dimensions 1, 2, 3 and the golden ratio and blocks 3 x 5, 1 x 1, 17 x 9 and
40 x 40 -- one block below a granule of the pools, one of a single element, one that ends inside a granule, one of several
granules.  The operator X -> A X B with A and B Hermitian per sector is Hermitian in the weighted inner product."""
import copy

import numpy as np

import tree_krylov_ref as ref
from cyten_amd import fusion_tree as ft
from cyten_amd import krylov
from tree_ops_cases import NumpyTreeBackend

PHI = (1.0 + np.sqrt(5.0)) / 2.0
QDIMS = (1.0, 2.0, 3.0, PHI)
ROWS = (3, 1, 17, 40)
COLS = (5, 1, 9, 40)
SHAPES = list(zip(ROWS, COLS))


class NumpyKrylovBackend(NumpyTreeBackend):
    """the stand-in of the tree operations + ``transform_blocks`` and the norm of complex blocks"""

    def transform_blocks(self, old_blocks, new_shapes, updates):
        from oracle import block_ops as ops
        return ops.transform_blocks(old_blocks, new_shapes, updates)

    def norm_many(self, blocks):
        return float(np.sqrt(sum(np.vdot(b, b).real for b in blocks)))


def spaces(qdims=QDIMS):
    """(codomain, domain): one tree per coupled sector"""
    sec = [[k] for k in range(len(ROWS))]
    q = np.array(qdims, dtype=np.float64)
    cod = ft.TreeSpace.from_multiplicities(sec, [[(r,)] for r in ROWS], q, 1, [[('r', k)] for k in range(len(ROWS))],
                                           [[(k,)] for k in range(len(ROWS))])
    dom = ft.TreeSpace.from_multiplicities(sec, [[(c,)] for c in COLS], q, 1, [[('c', k)] for k in range(len(COLS))],
                                           [[(k,)] for k in range(len(COLS))])
    return cod, dom


def _hermitian(rng, n, cplx, special=None):
    """eigenvalues in [0.5, 1.5], one of them replaced by `special`"""
    ev = rng.uniform(0.5, 1.5, n)
    if special is not None:
        ev[0] = special
    z = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0)
    q = np.linalg.qr(z)[0]
    h = (q * ev) @ q.conj().T
    return 0.5 * (h + h.conj().T)


def operator_blocks(rng, cplx):
    """(A, B) per sector.  The spectrum of X -> A X B is {lambda_i(A_c) mu_j(B_c)}: within [-3.75, 3.75] but for the
    non-degenerate lowest eigenvalue 2.5 * (-2.5) of the last sector -- a gap that lets 20-30 Lanczos steps converge"""
    last = len(ROWS) - 1
    A = [_hermitian(rng, r, cplx, 2.5 if k == last else None) for k, r in enumerate(ROWS)]
    B = [_hermitian(rng, c, cplx, -2.5 if k == last else None) for k, c in enumerate(COLS)]
    return A, B


def vector_blocks(rng, cplx):
    return [rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if cplx else 0) for sh in SHAPES]


def tree_tensor(bb, blocks, cod, dom):
    """one block per coupled sector (None: absent)"""
    rows = [(k, k) for k, b in enumerate(blocks) if b is not None]
    return ft.TreeTensor(ft.FusionTreeData(rows, [bb.as_block(b) for b in blocks if b is not None]), cod, dom)


def host_blocks(bb, t, shapes=SHAPES):
    """the blocks of a TreeTensor on the diagonal pairs (k, k) as numpy arrays, zeros where it has none"""
    have = {tuple(r): np.asarray(bb.to_numpy(b)) for r, b in zip(t.block_inds.tolist(), t.blocks)}
    assert all(i == j for i, j in have)
    return [have.get((k, k), np.zeros(sh)) for k, sh in enumerate(shapes)]


def chain(bb, A, B, cod, dom):
    """X -> A X B as a TreeChainOperator"""
    ta = tree_tensor(bb, A, cod, cod)
    tb = tree_tensor(bb, B, dom, dom)
    return krylov.TreeChainOperator(bb, [('compose_left', ta), ('compose_right', tb)], cod, dom)


class Case:
    """operator, start vector and their dense forms in scaled coordinates"""

    def __init__(self, bb, seed=0, cplx_op=False, cplx_vec=False, qdims=QDIMS):
        rng = np.random.default_rng(100 + seed)
        self.bb, self.qdims = bb, qdims
        self.cod, self.dom = spaces(qdims)
        self.A, self.B = operator_blocks(rng, cplx_op)
        self.x0 = vector_blocks(rng, cplx_vec)
        self.H = chain(bb, self.A, self.B, self.cod, self.dom)
        self.psi0 = tree_tensor(bb, self.x0, self.cod, self.dom)
        self.M = ref.dense_operator(self.A, self.B)
        self.y0 = ref.scaled(self.x0, qdims)

    def y(self, t):
        return ref.scaled(host_blocks(self.bb, t), self.qdims)

    def tensor(self, y):
        return tree_tensor(self.bb, ref.unscaled(y, SHAPES, self.qdims), self.cod, self.dom)


def check_ground_state(case, opts, flat=None):
    """the Lanczos criteria of tests/test_krylov.py:138-140 + the tridiagonal matrix against the dense Lanczos.  Returns
    the solver (after its run)."""
    bb = case.bb
    o = dict(opts, reortho=True)
    if flat is not None:
        o['flat'] = flat
    solver = krylov.LanczosGroundState(bb, case.H, case.psi0, o)
    E0, psi, N = solver.run()
    E, U = np.linalg.eigh(case.M)
    assert abs(E0 - E[0]) < 1e-9 * abs(E[0])
    assert abs(abs(np.vdot(U[:, 0], case.y(psi))) - 1.0) < 1e-7
    assert abs(ft.norm(bb, psi.data, psi.codomain) - 1.0) < 1e-12
    h = solver._h[:N + 1, :N + 1]
    want = ref.lanczos_h(case.M, case.y0, N)
    assert np.abs(h - want).max() <= 1e-10 * np.abs(want).max()
    return solver, N


# ---------------------------------------------------------------------------------------------------------------------------
# a chain with a leg move: abelian trees, where everything has a dense form

def braid_chain(bb, rng, cplx, perm_c=(2, 0, 1), perm_d=(1, 0)):
    """(operator, input TreeTensor, expected blocks as {(i, j): array}): X -> A X, a braid of the legs, -> X B with
    charge-conserving dense A and B on abelian trees (tests/fusion_tree_cases.py)"""
    from fusion_tree_cases import AbelianTrees
    at = AbelianTrees(rng)
    J, K = at.J, at.K
    T = at.dense(rng, cplx)
    cf, df = list(range(J)), list(range(J, J + K))
    cod, dom, data = at.to_blocks(T, cf, df)
    codomain_idcs, domain_idcs, ncf, ndf, mapping = at.braid(perm_c, perm_d)
    # A on (codomain, codomain)
    at_a = copy.copy(at)
    at_a.legs, at_a.J, at_a.K = [at.legs[f] for f in cf] * 2, J, J
    Ad = at_a.dense(rng, cplx)
    cod_a, dom_a, A = at_a.to_blocks(Ad, list(range(J)), list(range(J, 2 * J)))
    # B on (new domain, new domain)
    at_b = copy.copy(at)
    at_b.legs, at_b.J, at_b.K = [at.legs[f] for f in ndf] * 2, K, K
    Bd = at_b.dense(rng, cplx)
    cod_b, dom_b, B = at_b.to_blocks(Bd, list(range(K)), list(range(K, 2 * K)))
    ncod, ndom = at.space(ncf), at.space(ndf)
    dev = lambda d: ft.FusionTreeData(d.block_inds, [bb.as_block(b) for b in d.blocks])
    op = krylov.TreeChainOperator(bb, [('compose_left', ft.TreeTensor(dev(A), cod_a, dom_a)),
                                       ('transform', ncod, ndom, codomain_idcs, domain_idcs, mapping),
                                       ('compose_right', ft.TreeTensor(dev(B), cod_b, dom_b))], cod, dom)
    E = np.tensordot(Ad, T, axes=(list(range(J, 2 * J)), list(range(J))))
    E = np.transpose(E, list(perm_c) + [J + p for p in perm_d])
    E = np.tensordot(E, Bd, axes=(list(range(J, J + K)), list(range(K))))
    _, _, want = at.to_blocks(E, ncf, ndf)
    return op, ft.TreeTensor(dev(data), cod, dom), {tuple(r): b for r, b in zip(want.block_inds.tolist(), want.blocks)}, (ncod, ndom)


# ---------------------------------------------------------------------------------------------------------------------------
# the SU(2) x U(1) structure of tests/golden/su2_chi512.npz

def su2xu1_spaces(z, chi):
    """(codomain, domain) with the 28 coupled sectors (U(1) charge, 2j) of the golden file: the codomain is (bond leg, site,
    site) with its fusion trees -- a tree's rows are the multiplicity of its bond-leg sector scaled by chi / 512 -- and the
    domain one leg with as many columns per coupled sector as the codomain has rows; quantum dimensions 2j + 1"""
    f = chi / int(z['chi'])
    mult = {tuple(s): max(1, int(round(int(m) * f))) for s, m in zip(z['h_sectors'].tolist(), z['h_mults'].tolist())}
    by_key: dict = {}
    for r in sorted(z['h_rows_old'].tolist(), key=lambda r: (r[0], r[1], r[-2])):
        by_key.setdefault((r[0], r[1]), []).append(r)
    keys = sorted(by_key)
    mults = [[(mult[(r[2], r[3])], 1, 1) for r in by_key[k]] for k in keys]
    names = [[tuple(r[:-2]) for r in by_key[k]] for k in keys]
    qd = np.array([k[1] + 1.0 for k in keys])
    cod = ft.TreeSpace.from_multiplicities(keys, mults, qd, 3, names)
    dom = ft.TreeSpace.from_multiplicities(keys, [[(int(cod.block_size(i)),)] for i in range(len(keys))], qd, 1,
                                           [[('d', k)] for k in keys])
    return cod, dom
