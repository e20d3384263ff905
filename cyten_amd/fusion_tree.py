"""Host side of the non-abelian path: the block-backend callers of the reference's ``FusionTreeBackend`` on its own
data structure.

The symmetry layer -- fusion trees, F / R / B symbols, `TreePairMapping::from_instructions` -- is integer and symbol algebra
that never touches block data and stays what it is in the reference ("host-side fusion-tree bookkeeping stays").  What this
module mirrors is everything BETWEEN that layer and the block backend:

* :class:`FusionTreeData`  <- ``FusionTreeData`` (include/cyten/backends/fusion_tree_backend.h): one 2-D block per coupled
  sector, ``block_inds[n] = (i, j)``: index of the coupled sector in the codomain's / domain's ``sector_decomposition``.
* :class:`TreeSpace`  <- the part of ``TensorProduct`` the callers read: ``sector_decomposition``, ``block_size(i)``
  (``tp_mults``), ``sector_qdims``, ``iter_tree_blocks`` / ``tree_block_slice`` (which rows of a coupled block belong to which
  fusion tree, and the multiplicities of its uncoupled sectors).
* :func:`compose`  <- ``FusionTreeBackend::compose`` (src/backends/fusion_tree_backend.cpp:669-698): one ``matrix_dot`` per
  common coupled sector, no accumulation -- here ONE grouped launch.
* :func:`svd` / :func:`qr` / :func:`lq` / :func:`eigh`  <- ``::svd`` (:2184-2252), ``::qr`` (:2125-2180), ``::lq`` (:2070-2123),
  ``::eigh`` (:2033-2067): one batched decomposition over the present blocks, slices of the identity for the sectors
  without a block.
* :func:`truncate_singular_values`  <- ``::truncate_singular_values`` (:2254-2340): the selection of
  tensor_backend.cpp:139-242 with the marginal errors weighted by the sector's quantum dimension -- on the device
  (``cyb_truncate_select_weighted_f64``), the host sees counts, err and new_norm.
* :func:`transform_tensor`  <- ``TreePairMapping::transform_tensor`` (src/backends/fusion_tree_mapping.cpp:391-513), the body
  of ``FusionTreeBackend::apply_instructions`` (:593-631): the mapping (coefficients between tree pairs) comes from the
  symmetry layer as data; the loops over coupled sectors and tree pairs are the reference's, but instead of ``zeros`` +
  (``get_item``, ``mul``, ``operator+``) per term + ``permute_combined_matrix`` + ``set_item`` per tree pair they fill ONE
  descriptor list for ``HipBlockBackend.transform_blocks`` (one zero fill + one launch per tensor, complex coefficients).
* :func:`transform_tensor_factorized`  <- ``FactorizedTreeMapping::transform_tensor`` (fusion_tree_mapping.cpp:728-792) with
  ``transform_splitting_trees`` (:627-674) and ``transform_fusion_trees`` (:676-725), the other route of ``apply_instructions``
  (braids and twists inside each side): one sparse map over the splitting trees of the codomain, one over the fusion trees of
  the domain.  One strip record per new tree and one term per old tree that feeds it; the arithmetic is ONE
  ``tree_strip_many`` launch per side that is no identity, into blocks that are not zero-filled.
* :func:`inner` / :func:`trace_full` / :func:`norm`  <- ``::inner`` (:1238-1259), ``::trace_full`` (:1261-1278), ``::norm``
  (:1280-1296): ONE quantum-dimension weighted reduction (``inner_weighted_many`` / ``trace_weighted_many``) instead of a
  reduction and a host wait per coupled sector.  :func:`mul`, :func:`linear_combination`, :func:`dagger`,
  :func:`almost_equal`  <- ``::mul`` (:1298-1314), ``::linear_combination`` (:1316-1360), ``::dagger`` (:717-729),
  ``::almost_equal`` (:560-590).
* :func:`scale_axis`  <- ``::scale_axis`` (:3521-3644), :func:`mask_contract`  <- ``::_mask_contract`` (:2372-2500): the loops
  over forest blocks emit one :class:`TreeAxisRecord` per tree block; the arithmetic is ONE ``tree_axis_many`` launch.  Both are
  defined PER TREE BLOCK (rows ``start:stop`` of a tree, reshaped to its multiplicities in C order), which is what
  ``iter_tree_blocks`` and ``transform_tensor`` mean; the reference's ``_mask_contract`` reshapes a codomain forest to
  ``(m..., -1)`` (:2471), which mixes the tree index into the columns when a forest holds several trees, and is not reproduced.
* :func:`truncated_svd`: svd, truncation and the mask on U, S and Vh -- three launches after the SVD.
* :func:`partial_trace`  <- ``::partial_trace`` (:2883-3183): step 1 is :func:`transform_tensor`; the loops of step 2
  (:3092-3159, seven block-backend calls per tree pair) emit one output record per tile of the result blocks and one weighted
  term per contributing old tree pair; the arithmetic is ONE ``tree_trace_many`` launch.  The per-tree data of the symmetry
  layer (``partial_trace_helper`` :2557-2604, the new trees) comes in as a :class:`TreeTrace`.
* :func:`outer`  <- ``::outer`` (:2609-2667): the double loop over the tree-block pairs of a and of b emits one output record
  per tile of the result blocks and one weighted term per contributing (a tree pair, b tree pair); the arithmetic is ONE
  ``tree_outer_many`` launch.  What ``FusionTree::outer`` says per pair of trees comes in as a :class:`TreeOuter`.
* :func:`partial_compose`  <- ``::partial_compose`` (:2670-2880): the five-deep loop over outer trees, b's codomain trees, b's
  domain trees, old trees and new trees emits one output record per new tree of the contracted side (a strip of a result
  block) and one weighted term per innermost iteration; the arithmetic is ONE ``tree_compose_many`` launch.  What
  ``FusionTree::insert_at`` says per (outer tree, tree of b) comes in as a :class:`TreeInsert`.
* :func:`to_dense_block`  <- ``::to_dense_block`` (:1856-1973) with ``_get_forest_block_contribution`` (:1532-1604): the loops over
  blocks, forest pairs and tree pairs emit one region record per combination of leg sectors (the regions partition the dense
  tensor, so nothing is zero-filled) and one term per (block, tree, tree) whose weight is a small tensor, the contracted pair
  of tree tensors; the arithmetic is ONE ``tree_to_dense_many`` launch.  What ``FusionTree::to_dense_block`` and
  ``batch_sector_dim`` say per tree and per sector comes in as a :class:`TreeDense`.
* :func:`from_dense_block`  <- ``::from_dense_block`` (:1680-1853) with ``_add_forest_block_entries`` (:1606-1677): one output
  record per (tree, tree) tile of every common coupled sector, the dense block read in place; the projection is ONE
  ``tree_from_dense_many`` launch, the tolerance check one weighted :func:`norm` and one norm of the dense block.
* :func:`from_grid`  <- ``::from_grid`` (:3375-3518, under ``tensor_from_grid``): the direct sum of a grid of tree tensors along
  ``codomain[0]`` (rows) and ``domain[-1]`` (columns) -- an MPO tensor from operators, the sum of two MPS, a subspace expansion.
  Every (new codomain tree, new domain tree) tile is partitioned into the cells of the grid; a cell an entry feeds is one copy
  record of the entry's own tile read in place under the cell's factor, every other cell a record of zeros; the arithmetic is
  ONE ``tree_place_many`` launch that writes every element of the result once (no zero fill, no promotion pass, no ``mul``
  per factor).  The new spaces and the cumulative multiplicity tables come in as data; trees are matched by key.
* :func:`from_tree_pairs`  <- ``::from_tree_pairs`` (:3186-3263): blocks ``(m_1 .. m_J, n_K .. n_1)`` per pair of trees into their
  tiles, the permutation and the reshape done by the strides of ONE ``tree_place_many`` launch.  :func:`eye`  <- ``::eye_data``
  (:1180-1192).
* :class:`TreeTensor`: data + codomain + domain, the vector the Krylov solvers and the operator wrappers take
  (``cyten_amd.krylov``, ``cyten_amd.sparse``): the reference's Krylov code calls ``inner`` / ``norm`` /
  ``linear_combination`` on whatever tensor it is given (src/tensors/krylov_based.cpp), and those need the quantum dimensions
  of the codomain, which :class:`FusionTreeData` alone does not carry.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

__all__ = ['TreeBlock', 'TreeSpace', 'FusionTreeData', 'compose', 'svd', 'qr', 'lq', 'eigh', 'truncate_singular_values',
           'transform_tensor', 'transform_tensor_factorized', 'discard_zero_blocks', 'norm', 'inner', 'trace_full', 'mul', 'linear_combination', 'dagger',
           'almost_equal', 'TreeAxisRecord', 'TreeMask', 'leg_keys', 'scale_axis', 'mask_contract', 'truncated_svd', 'TreeTensor',
           'same_space', 'TreeTrace', 'partial_trace', 'TreeOuter', 'outer', 'TreeInsert', 'partial_compose',
           'TreeDense', 'to_dense_block', 'from_dense_block', 'from_grid', 'from_tree_pairs', 'eye']


@dataclass(frozen=True)
class TreeBlock:
    """one fusion tree of a coupled sector: its rows inside the coupled block and the multiplicities of its uncoupled
    sectors (``TreeBlockInfo`` of ``TensorProduct::iter_tree_blocks``: tree, slice, multiplicities)"""
    tree: object           # hashable identifier of the fusion tree (the symmetry layer's FusionTree, or any key)
    start: int
    stop: int
    multiplicities: tuple
    uncoupled: tuple = ()  # one hashable sector key per flat leg (``TreeBlockInfo::uncoupled``); () where the caller has none


@dataclass
class TreeSpace:
    """What the block path reads of a ``TensorProduct``: sorted coupled sectors, block size and quantum dimension of each,
    and the tree blocks inside each coupled sector (in ``iter_tree_blocks`` order)."""
    sectors: np.ndarray            # (n_coupled, n_sym) int64: sector_decomposition, lexsorted
    qdims: np.ndarray              # (n_coupled,) sector_qdims
    tree_blocks: list              # per coupled sector: [TreeBlock, ...] with contiguous ascending slices
    num_legs: int = 0              # num_flat_legs
    _where: dict = field(default_factory=dict, repr=False)

    def __post_init__(self):
        self.sectors = np.asarray(self.sectors, dtype=np.int64).reshape(len(self.tree_blocks), -1)
        self.qdims = np.asarray(self.qdims, dtype=np.float64)
        self._where = {}
        for i, tbs in enumerate(self.tree_blocks):
            for tb in tbs:
                self._where[tb.tree] = (i, tb)

    @property
    def num_sectors(self):
        return len(self.tree_blocks)

    @property
    def multiplicities(self) -> np.ndarray:
        """block_size(i) of every coupled sector (``tp_mults``)"""
        return np.array([tbs[-1].stop if tbs else 0 for tbs in self.tree_blocks], dtype=np.int64)

    def block_size(self, i: int) -> int:
        tbs = self.tree_blocks[i]
        return tbs[-1].stop if tbs else 0

    def has_tree(self, tree) -> bool:
        return tree in self._where

    def tree_block_slice(self, tree):
        """(coupled sector index, TreeBlock) of a tree (``tree_block_slice`` + the tree's ``coupled``)"""
        return self._where[tree]

    @classmethod
    def from_multiplicities(cls, sectors, tree_mults, qdims=None, num_legs=0, names=None, uncoupled=None):
        """``tree_mults[i]``: list of multiplicity tuples of the trees of coupled sector i (block rows in that order);
        ``uncoupled[i][t]``: the sector keys of the legs of tree t, where the caller has them"""
        blocks = []
        for i, lst in enumerate(tree_mults):
            off, tbs = 0, []
            for t, m in enumerate(lst):
                m = tuple(int(x) for x in m)
                sz = int(np.prod(m)) if m else 1
                tbs.append(TreeBlock(names[i][t] if names is not None else (i, t), off, off + sz, m,
                                     tuple(uncoupled[i][t]) if uncoupled is not None else ()))
                off += sz
            blocks.append(tbs)
        q = np.ones(len(blocks)) if qdims is None else qdims
        return cls(sectors, q, blocks, num_legs)


def common_sectors(a: TreeSpace, b: TreeSpace):
    """(i, j) of the coupled sectors both spaces hold, ascending (``iter_common_sorted_arrays`` of the two sorted
    ``sector_decomposition``s)"""
    where = {tuple(s): j for j, s in enumerate(b.sectors.tolist())}
    return [(i, where[tuple(s)]) for i, s in enumerate(a.sectors.tolist()) if tuple(s) in where]


@dataclass
class FusionTreeData:
    block_inds: np.ndarray     # (n_blocks, 2), lexsorted, duplicate free
    blocks: list

    def __post_init__(self):
        self.block_inds = np.asarray(self.block_inds, dtype=np.int64).reshape(len(self.blocks), 2)

    def sorted(self) -> 'FusionTreeData':
        order = np.lexsort(self.block_inds.T) if len(self.blocks) else np.zeros(0, dtype=np.int64)
        return FusionTreeData(self.block_inds[order], [self.blocks[i] for i in order])

    def block_ind_from_domain_sector(self, j: int):
        """index of the block whose domain sector index is j (``block_ind_from_coupled``), or None"""
        hit = np.flatnonzero(self.block_inds[:, 1] == j)
        return int(hit[0]) if len(hit) else None


@dataclass
class TreeTensor:
    """A fusion-tree tensor as a vector: its blocks and the two spaces that give them a meaning -- the quantum dimensions of
    ``codomain`` weight :func:`inner` and :func:`norm`.  ``blocks`` / ``block_inds`` forward to ``data``."""
    data: FusionTreeData
    codomain: TreeSpace
    domain: TreeSpace

    @property
    def blocks(self) -> list:
        return self.data.blocks

    @property
    def block_inds(self) -> np.ndarray:
        return self.data.block_inds

    def like(self, data: FusionTreeData) -> 'TreeTensor':
        """`data` on the spaces of this tensor"""
        return TreeTensor(data, self.codomain, self.domain)


def same_space(a: TreeSpace, b: TreeSpace) -> bool:
    """the same coupled sectors with the same block sizes: blocks on `a` can be added to, or contracted with, blocks on `b`"""
    return a is b or (np.array_equal(a.sectors, b.sectors) and np.array_equal(a.multiplicities, b.multiplicities))


# ---------------------------------------------------------------------------------------------------------------------------

def compose(bb, a: FusionTreeData, b: FusionTreeData) -> FusionTreeData:
    """fusion_tree_backend.cpp:669-698: blocks of a and b that share the coupled sector (a's domain index == b's codomain
    index) are multiplied, nothing is accumulated.  One grouped launch for the tensor."""
    ja = {int(j): n for n, j in enumerate(a.block_inds[:, 1])}
    groups, rows = [], []
    for m, i in enumerate(b.block_inds[:, 0]):
        n = ja.get(int(i))
        if n is not None:
            groups.append([(a.blocks[n], b.blocks[m])])
            rows.append((int(a.block_inds[n, 0]), int(b.block_inds[m, 1])))
    if not groups:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    return FusionTreeData(np.array(rows, dtype=np.int64), bb.matrix_dot_grouped(groups)).sorted()


def _eye_slice(bb, dim, rows, cols, like):
    eye = bb.eye_matrix(int(dim), dtype=getattr(like, 'dtype', None))
    return bb.get_item(eye, (slice(0, rows) if rows is not None else slice(None), slice(0, cols) if cols is not None else slice(None)))


def _decompose(bb, a: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, new_mults, kind, arg=None):
    """shared loop of ::svd / ::qr / ::lq: every common coupled sector gets its isometries, the sectors without a block from
    the identity; ONE batched call for the present blocks"""
    common = common_sectors(codomain, domain)
    have = {int(i): n for n, i in enumerate(a.block_inds[:, 0])}
    cm, dm = codomain.multiplicities, domain.multiplicities
    if new_mults is None:
        new_mults = [min(int(cm[i]), int(dm[j])) for i, j in common]
    present = [(k, i, j) for k, (i, j) in enumerate(common) if i in have]
    srcs = [a.blocks[have[i]] for _, i, _ in present]
    like = srcs[0] if srcs else None
    if kind == 'svd':
        facs = bb.matrix_svd_batched(srcs, arg) if srcs else []
    elif kind == 'qr':
        facs = bb.matrix_qr_batched(srcs, False) if srcs else []
    else:
        facs = bb.matrix_lq_batched(srcs, False) if srcs else []
    it = iter(facs)
    done = {k for k, _, _ in present}
    return common, new_mults, done, it, like


def svd(bb, a: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, new_mults=None, algorithm=None):
    """fusion_tree_backend.cpp:2184-2252.  Returns (U, S, Vh) as FusionTreeData with block_inds (i_cod, i_new), (i_new, i_new),
    (i_new, i_dom); S only for the sectors that have a block."""
    common, new_mults, done, it, like = _decompose(bb, a, codomain, domain, new_mults, 'svd', algorithm)
    cm, dm = codomain.multiplicities, domain.multiplicities
    ub, ur, sb, sr, vb, vr = [], [], [], [], [], []
    for k, (i, j) in enumerate(common):
        ur.append((i, k))
        vr.append((k, j))
        if k in done:
            u, s, vh = next(it)
            ub.append(u), sb.append(s), vb.append(vh)
            sr.append((k, k))
        else:
            ub.append(_eye_slice(bb, cm[i], None, int(new_mults[k]), like))
            vb.append(_eye_slice(bb, dm[j], int(new_mults[k]), None, like))
    return FusionTreeData(ur, ub), FusionTreeData(sr, sb), FusionTreeData(vr, vb)


def qr(bb, a: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, new_mults=None):
    """fusion_tree_backend.cpp:2125-2180: (Q with rows (i_cod, i_new), R with rows (i_new, i_dom))"""
    common, new_mults, done, it, like = _decompose(bb, a, codomain, domain, new_mults, 'qr')
    cm = codomain.multiplicities
    qb, qrw, rb, rr = [], [], [], []
    for k, (i, j) in enumerate(common):
        qrw.append((i, k))
        if k in done:
            q, r = next(it)
            qb.append(q), rb.append(r)
            rr.append((k, j))
        else:
            qb.append(_eye_slice(bb, cm[i], None, int(new_mults[k]), like))
    return FusionTreeData(qrw, qb), FusionTreeData(rr, rb)


def lq(bb, a: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, new_mults=None):
    """fusion_tree_backend.cpp:2070-2123: (L with rows (i_cod, i_new), Q with rows (i_new, i_dom))"""
    common, new_mults, done, it, like = _decompose(bb, a, codomain, domain, new_mults, 'lq')
    dm = domain.multiplicities
    lb, lr, qb, qrw = [], [], [], []
    for k, (i, j) in enumerate(common):
        qrw.append((k, j))
        if k in done:
            l, q = next(it)
            lb.append(l), qb.append(q)
            lr.append((i, k))
        else:
            qb.append(_eye_slice(bb, dm[j], int(new_mults[k]), None, like))
    return FusionTreeData(lr, lb), FusionTreeData(qrw, qb)


def eigh(bb, a: FusionTreeData, codomain: TreeSpace, sort=None):
    """fusion_tree_backend.cpp:2033-2067: (W, V); a sector without a block has eigenvalues 0 (no W block) and the standard
    basis as eigenvectors"""
    have = {int(i): n for n, i in enumerate(a.block_inds[:, 0])}
    srcs = [a.blocks[have[i]] for i in sorted(have)]
    res = iter(bb.eigh_batched(srcs, sort) if srcs else [])
    like = srcs[0] if srcs else None
    vb, wb = [], []
    for i in range(codomain.num_sectors):
        if i in have:
            w, v = next(res)
            wb.append(w), vb.append(v)
        else:
            vb.append(bb.eye_matrix(codomain.block_size(i), dtype=getattr(like, 'dtype', None)))
    return (FusionTreeData(a.block_inds[np.argsort(a.block_inds[:, 0], kind='stable')].copy(), wb),
            FusionTreeData([(i, i) for i in range(codomain.num_sectors)], vb))


def truncate_singular_values(bb, S: FusionTreeData, domain: TreeSpace, **options):
    """fusion_tree_backend.cpp:2254-2340: every sector of the new leg contributes ``multiplicities[j]`` values (zeros where S
    has no block) weighted by ``sector_qdims[j]``.  Returns (mask_blocks, mask_block_inds, err, new_norm): boolean host
    vectors of the sectors that keep at least one value, rows (small index, large index j), as the reference builds its
    Mask.  The selection runs on the device when the backend offers it (weights are one number per sector)."""
    return _truncate(bb, S, domain, **options)[:4]


def _truncate(bb, S: FusionTreeData, domain: TreeSpace, **options):
    """:func:`truncate_singular_values` + the kept positions per sector j as the device tables of ``truncate_select``
    (``{j: DeviceIndex}``), or None where the selection ran on the host"""
    mults = [int(m) for m in domain.multiplicities]
    have = {int(i): n for n, i in enumerate(S.block_inds[:, 0])}
    absent = [j for j in range(len(mults)) if j not in have and mults[j] > 0]
    zeros = iter(bb.zeros_many([(mults[j],) for j in absent])) if absent else iter(())
    blocks = []
    for j, m in enumerate(mults):
        if m == 0:
            continue
        blocks.append(S.blocks[have[j]] if j in have else next(zeros))
    sec = [j for j, m in enumerate(mults) if m > 0]
    q = np.array([domain.qdims[j] for j in sec], dtype=np.float64)
    if hasattr(bb, 'truncate_select') and 0 < sum(mults) <= bb.TRUNCATE_MAX:
        tables, mask, err, new_norm = bb.truncate_select(blocks, qdims=q, **options)
        keep = bb.to_numpy(mask).astype(bool)
        tables = dict(zip(sec, tables))
    else:
        tables = None
        from . import abelian as ab
        S_np = np.concatenate([bb.to_numpy(b) for b in blocks]) if blocks else np.zeros(0)
        keep, err, new_norm = ab.truncation_selection(S_np, qdims=np.repeat(q, [mults[j] for j in sec]), **options)
    out_b, out_r, off = [], [], 0
    for j in sec:
        blk = keep[off:off + mults[j]]
        off += mults[j]
        if blk.any():
            out_r.append((len(out_r), j))
            out_b.append(blk.copy())
    return out_b, np.array(out_r, dtype=np.int64).reshape(len(out_r), 2), float(err), float(new_norm), tables


def norm(bb, a: FusionTreeData, codomain: TreeSpace) -> float:
    """fusion_tree_backend.cpp:1283-1297: sqrt(sum_n qdim(coupled_n) |block_n|^2), one reduction per block list -- with
    different quantum dimensions the weighted one, where the backend has it"""
    if not a.blocks:
        return 0.0
    q = codomain.qdims[a.block_inds[:, 0]]
    if np.all(q == q[0]):
        return float(np.sqrt(q[0]) * bb.norm_many(a.blocks))
    if hasattr(bb, 'inner_weighted_many'):
        return float(np.sqrt(bb.inner_weighted_many(a.blocks, None, q)))
    return float(np.sqrt(sum(float(qi) * bb.norm_many([b]) ** 2 for qi, b in zip(q, a.blocks))))


# ---------------------------------------------------------------------------------------------------------------------------

def transform_tensor(bb, data: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, new_codomain: TreeSpace, new_domain: TreeSpace,
                     codomain_idcs, domain_idcs, mapping) -> FusionTreeData:
    """``TreePairMapping::transform_tensor`` (fusion_tree_mapping.cpp:391-513).  `mapping`: the data of the symmetry layer's
    TreePairMapping, ``{(old codomain tree, old domain tree): {(new codomain tree, new domain tree): coefficient}}``
    (``mapping.data[I][J]``, f(T)_{Jm} = sum_I mapping[I][J] T_{Im}, :401).  `codomain_idcs` / `domain_idcs`: which old legs
    (numbered codomain first, then the domain legs counted from the end, :415-431) make up the new codomain / domain.

    Loops as in the reference -- common coupled sectors of the new spaces (:441-450), new tree-block pairs (:453-454), the old
    tree pairs that feed them (:456-478), old multiplicities in the new axis order (:484-499) -- but what they emit is one
    update record per new tree pair; the arithmetic is ONE ``transform_blocks`` call.  The result is complex if the data or a
    coefficient is (:433-436)."""
    J, K = codomain.num_legs, domain.num_legs
    N = J + K
    axes1 = [i if i < J else (N - 1) + (J - i) for i in codomain_idcs]
    axes2 = [i if i < J else (N - 1) + (J - i) for i in domain_idcs]
    leg_perm = list(codomain_idcs) + list(domain_idcs)[::-1]
    inv_leg_perm = [0] * len(leg_perm)
    for pos, src in enumerate(leg_perm):
        inv_leg_perm[src] = pos
    by_new: dict = {}        # (new tree pair) -> [(old codomain tree, old domain tree, coefficient)]
    for (t1, t2), targets in mapping.items():
        for new_pair, coeff in targets.items():
            by_new.setdefault(new_pair, []).append((t1, t2, coeff))
    block_of_dom = {int(j): n for n, j in enumerate(data.block_inds[:, 1])}
    new_rows, shapes, updates = [], [], []
    for i, j in common_sectors(new_codomain, new_domain):
        ups = []
        for xb in new_codomain.tree_blocks[i]:
            for yb in new_domain.tree_blocks[j]:
                srcs = by_new.get((xb.tree, yb.tree))
                if not srcs:
                    continue
                terms = []
                for t1, t2, coeff in srcs:
                    _, b1 = codomain.tree_block_slice(t1)
                    jd, b2 = domain.tree_block_slice(t2)
                    n = block_of_dom.get(jd)
                    if n is None:          # the old tensor has no block in that coupled sector
                        continue
                    terms.append((coeff, n, (b1.start, b1.stop), (b2.start, b2.stop)))
                if not terms:
                    continue
                leg_mults = list(xb.multiplicities) + list(yb.multiplicities)[::-1]
                old_mults = [leg_mults[k] for k in inv_leg_perm]
                ups.append((len(shapes), (xb.start, xb.stop), (yb.start, yb.stop), old_mults[:J], axes1, old_mults[J:][::-1], axes2, terms))
        if not ups:
            continue                       # (is_zero_block, :509-511)
        updates += ups
        new_rows.append((i, j))
        shapes.append((new_codomain.block_size(i), new_domain.block_size(j)))
    if not shapes:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    return FusionTreeData(np.array(new_rows, dtype=np.int64), bb.transform_blocks(data.blocks, shapes, updates))


MAX_STRIP_LEGS = 6      # flat legs of one side of a factorized move (the levels of a strip, CYB_TREE_PLACE_MAX_LEVELS)


def _strip_records(live, blocks, side: int, old_space: TreeSpace, new_space: TreeSpace, axes, table, name: str):
    """the loops of ``transform_splitting_trees`` (side 0, fusion_tree_mapping.cpp:627-674) / ``transform_fusion_trees`` (side 1,
    :676-725) over the sectors `live` = [(i, j)] whose current blocks are `blocks`: per sector the strip records of its new
    trees, ``(start, stop, mults_old_order, [(old start, coefficient)])`` with the terms in ascending order of the old tree's
    start, or None where no new tree of the sector has a term (the block is dropped, :773 / :780)"""
    what = 'codomain' if side == 0 else 'domain'
    if sorted(axes) != list(range(len(axes))) or len(axes) != new_space.num_legs:
        raise ValueError(f'{name}: the {what} axes {list(axes)} are no permutation of the {new_space.num_legs} legs of the new {what}')
    if len(axes) > MAX_STRIP_LEGS:
        raise ValueError(f'{name}: {len(axes)} {what} legs, at most {MAX_STRIP_LEGS} on a side')
    inv = [0] * len(axes)
    for pos, a in enumerate(axes):
        inv[a] = pos
    by_new: dict = {}        # new tree -> [(old tree, coefficient)]
    for old_tree, targets in table.items():
        for new_tree, coeff in targets.items():
            by_new.setdefault(new_tree, []).append((old_tree, coeff))
    old_sectors, new_sectors = old_space.sectors.tolist(), new_space.sectors.tolist()
    out = []
    for (i, j), blk in zip(live, blocks):
        s = (i, j)[side]
        sector = new_sectors[s]
        strips, fed = [], False
        for x2 in new_space.tree_blocks[s]:
            if len(x2.multiplicities) != len(axes):
                raise ValueError(f'{name}: the new {what} tree {x2.tree!r} has {len(x2.multiplicities)} multiplicities for {len(axes)} legs')
            mults_old = tuple(x2.multiplicities[k] for k in inv)
            terms = []
            for X, coeff in by_new.get(x2.tree, ()):
                if not old_space.has_tree(X):
                    raise ValueError(f'{name}: the old {what} holds no tree {X!r}')
                io, xb = old_space.tree_block_slice(X)
                if old_sectors[io] != sector:
                    raise ValueError(f'{name}: the old {what} tree {X!r} and the new tree {x2.tree!r} lie in different coupled sectors')
                if tuple(xb.multiplicities) != mults_old:
                    raise ValueError(f'{name}: the old {what} tree {X!r} has the multiplicities {tuple(xb.multiplicities)}, the new tree '
                                     f'{x2.tree!r} in the old leg order {mults_old}')
                if xb.stop > blk.shape[side]:
                    raise ValueError(f'{name}: the strip {xb.start}:{xb.stop} of the old {what} tree {X!r} does not fit its block of shape '
                                     f'{tuple(blk.shape)}')
                terms.append((xb.start, coeff))
            if x2.stop - x2.start != math.prod(mults_old) or x2.stop > new_space.block_size(s):
                raise ValueError(f'{name}: the strip {x2.start}:{x2.stop} of the new {what} tree {x2.tree!r} does not fit its multiplicities '
                                 f'{tuple(x2.multiplicities)} or its block of {new_space.block_size(s)}')
            terms.sort(key=lambda tm: tm[0])
            fed = fed or bool(terms)
            strips.append((x2.start, x2.stop, mults_old, terms))
        out.append(strips if fed else None)
    return out


def transform_tensor_factorized(bb, data: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, new_codomain: TreeSpace,
                                new_domain: TreeSpace, codomain_idcs, domain_idcs, splitting=None, fusion=None) -> FusionTreeData:
    """``FactorizedTreeMapping::transform_tensor`` (fusion_tree_mapping.cpp:728-792), the route of
    ``FusionTreeBackend::apply_instructions`` for moves that stay inside each side (braids and twists, no bends).  `splitting` /
    `fusion`: the data of the two halves of the symmetry layer's FactorizedTreeMapping, ``{old tree: {new tree: coefficient}}``
    over the splitting trees of the codomain / the fusion trees of the domain (``SparseMappingFusionTree::data``); None stands
    for the ``IdentityMappingFusionTree``.  `codomain_idcs`: a permutation of ``range(J)``, `domain_idcs`: one of ``range(J, N)``
    (numbered as for :func:`transform_tensor`).

    Loops as in the reference -- common coupled sectors of the new spaces, the old block through the coupled sector in the old
    domain (:762), per new tree of a side the old trees that feed it -- but what they emit is one strip record per new tree
    (its rows and all columns, or its columns and all rows) with one term per old tree, added in ascending order of the old
    tree's start; the arithmetic is ONE ``tree_strip_many`` launch per side that is no identity, into blocks from
    ``empty_many``: every element is written once, a new tree without a term as zeros, nothing is zero-filled.  A sector none
    of whose new trees has a term is dropped (:773, :780); with both sides None the result holds the old block objects.  The
    result is complex if the data or a coefficient is (:747-750); float64 data is then read as it stands."""
    name = 'transform_tensor_factorized'
    J, K = codomain.num_legs, domain.num_legs
    N = J + K
    codomain_idcs, domain_idcs = [int(i) for i in codomain_idcs], [int(i) for i in domain_idcs]
    if sorted(codomain_idcs) != list(range(J)) or sorted(domain_idcs) != list(range(J, N)):
        raise ValueError(f'{name}: codomain_idcs {codomain_idcs} / domain_idcs {domain_idcs} are no permutations of the {J} codomain / the '
                         f'{K} domain legs: a move that mixes the sides takes transform_tensor')
    axes2 = [(N - 1) - i for i in domain_idcs]                                        # (:741-745)
    old_dom = {tuple(sec): jd for jd, sec in enumerate(domain.sectors.tolist())}
    block_of_dom = {int(j): n for n, j in enumerate(data.block_inds[:, 1])}
    live, blocks = [], []
    for i, j in common_sectors(new_codomain, new_domain):
        n = block_of_dom.get(old_dom.get(tuple(new_codomain.sectors[i].tolist())))
        if n is not None:                                                             # (no old block: no result block, :763)
            live.append((i, j))
            blocks.append(data.blocks[n])
    cplx = any(_is_complex(b) for b in data.blocks) or any(
        complex(c).imag != 0 for table in (splitting, fusion) if table is not None for targets in table.values() for c in targets.values())
    dtype = np.complex128 if cplx else np.float64
    # both sides are planned and checked before anything is enqueued (the codomain pass keeps the columns of a block)
    passes = [(side, new_space, axes, _strip_records(live, blocks, side, old_space, new_space, axes, table, name))
              for side, old_space, new_space, axes, table in ((0, codomain, new_codomain, codomain_idcs, splitting),
                                                              (1, domain, new_domain, axes2, fusion)) if table is not None]
    keep = [k for k in range(len(live)) if all(plan[k] is not None for _, _, _, plan in passes)]          # (:773, :780)
    for k in keep:
        (i, j), sh = live[k], tuple(blocks[k].shape)
        want = (new_codomain.block_size(i) if splitting is not None else sh[0], new_domain.block_size(j) if fusion is not None else sh[1])
        if want != (new_codomain.block_size(i), new_domain.block_size(j)):
            raise ValueError(f'{name}: the old block of the coupled sector {new_codomain.sectors[i].tolist()} has the shape {sh}, the new '
                             f'spaces ask for {(new_codomain.block_size(i), new_domain.block_size(j))}: a strip does not fit its block')
    live, blocks = [live[k] for k in keep], [blocks[k] for k in keep]
    for side, new_space, axes, plan in passes:
        if not live:
            break
        shapes = [((new_space.block_size(i), b.shape[1]) if side == 0 else (b.shape[0], new_space.block_size(j))) for (i, j), b in zip(live, blocks)]
        outs = bb.empty_many(shapes, dtype=dtype)
        bb.tree_strip_many([(out, side, start, stop, mults_old, axes, [(src, s0, c) for s0, c in terms])
                            for out, src, k in zip(outs, blocks, keep) for start, stop, mults_old, terms in plan[k]])
        blocks = outs
    if not live:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    return FusionTreeData(np.array(live, dtype=np.int64), list(blocks))


def discard_zero_blocks(bb, data: FusionTreeData, eps: float) -> FusionTreeData:
    """``FusionTreeData::discard_zero_blocks`` after ``apply_instructions`` (fusion_tree_backend.cpp:629): blocks whose
    largest entry is at most `eps` are dropped -- ONE batched reduction decides for the whole tensor when the backend has one"""
    if not data.blocks:
        return data
    keep = [n for n, b in enumerate(data.blocks) if not bb.max_abs(b) <= eps]
    if len(keep) == len(data.blocks):
        return data
    return FusionTreeData(data.block_inds[keep], [data.blocks[n] for n in keep])


# ---------------------------------------------------------------------------------------------------------------------------
# partial trace

class TreeTrace(NamedTuple):
    """What the symmetry layer knows about tracing adjacent leg pairs of ONE side (codomain or domain), as data:
    ``partial_trace_helper`` (fusion_tree_backend.cpp:2557-2604: the ``on_diag`` flag and the product of conjugated B symbols and
    Frobenius-Schur signs) and the ``FusionTree`` constructions at :3109 / :3136, per tree."""
    positions: tuple   # ascending k, non-overlapping: legs (k, k+1) of THIS side (codomain order / domain order) are one traced pair
    table: dict        # old tree key -> (new tree key, factor); a tree that is absent is off the diagonal (on_diag == False)


def _traced_tree(space: TreeSpace, new_space: TreeSpace, trace, i_old: int, tb: TreeBlock, what: str):
    """(new TreeBlock, factor) of an old tree of a surviving coupled sector, or None if it is off the diagonal"""
    m = tb.multiplicities
    if trace is None:
        key, factor, positions = tb.tree, 1.0, ()
    else:
        positions = trace.positions
        if len(m) != space.num_legs or len(tb.uncoupled) != len(m) or any(k + 1 >= len(m) for k in positions):
            raise ValueError(f'partial_trace: a {what} tree lacks the uncoupled sector keys or the multiplicities of its legs '
                             '(TreeBlock.uncoupled, TreeBlock.multiplicities)')
        hit = trace.table.get(tb.tree)
        if hit is None:
            return None
        key, factor = hit
        for k in positions:
            if m[k] != m[k + 1]:
                raise ValueError(f'partial_trace: the legs {k} and {k + 1} of a {what} tree on the diagonal have the multiplicities '
                                 f'{m[k]} and {m[k + 1]}')
    if not new_space.has_tree(key):
        raise ValueError(f'partial_trace: the new {what} has no tree {key!r}')
    i_new, nb = new_space.tree_block_slice(key)
    dropped = {k for p in positions for k in (p, p + 1)}
    if tuple(nb.multiplicities) != tuple(x for a, x in enumerate(m) if a not in dropped):
        raise ValueError(f'partial_trace: the multiplicities {tuple(nb.multiplicities)} of a new {what} tree are not the old ones {tuple(m)} '
                         f'without the traced legs')
    if new_space.sectors[i_new].tolist() != space.sectors[i_old].tolist():
        raise ValueError(f'partial_trace: a new {what} tree lies in another coupled sector than the old one')
    return nb, factor


def partial_trace(bb, data: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, new_codomain: TreeSpace, new_domain: TreeSpace,
                  cod_trace: TreeTrace = None, dom_trace: TreeTrace = None, eps: float = 0.0, discard: bool = True, move=None) -> FusionTreeData:
    """``FusionTreeBackend::partial_trace`` (fusion_tree_backend.cpp:2883-3183).  `cod_trace` / `dom_trace`: which adjacent leg
    pairs of the codomain / domain are traced and what the symmetry layer says per tree (:class:`TreeTrace`); a side with None
    is not traced (factor 1, the same trees).  `new_codomain` / `new_domain`: the spaces after tracing (:2934-2948).

    `move = (mid_codomain, mid_domain, codomain_idcs, domain_idcs, mapping)` first runs :func:`transform_tensor` -- step 1
    (:2908-3025), which bends and braids the legs until every traced pair is adjacent on one side; the traces then refer to
    the mid spaces.  Two launches and a zero fill in total.

    Step 2 has the reference's loops -- a coupled sector of the data survives if both new spaces hold it (:3027-3047); old
    codomain trees on the diagonal, then old domain trees on the diagonal (:3092-3159) -- but what they emit is one output
    record per (new codomain tree, new domain tree) tile of every result block, tiles without a term included (they are
    written as zeros, so the result blocks need no zero fill), and one term record per contributing old tree pair with the
    coefficient ``f_cod * conj(f_dom)`` (:3149), ordered by ascending old codomain tree, then old domain tree.  The tile of
    an old tree pair is read in place, reshaped to (codomain multiplicities..., domain multiplicities...) (:3121-3142).  ONE
    ``tree_trace_many`` call.  Result blocks exist for the surviving sectors only (the reference allocates every common
    sector of the new spaces as zeros and discards them again, :3037, :3160); the result goes through
    :func:`discard_zero_blocks` with `eps` unless ``discard=False``, and is complex if the data or a factor is.

    With zero remaining legs on both sides (new spaces of zero legs: one coupled sector, one tree without multiplicities, block
    size 1) the result always is the single 1 x 1 block with ``block_inds`` (0, 0) and is not discarded (:3162-3181): the caller
    reads the scalar with ``bb.to_numpy(result.blocks[0])[0, 0]`` (one download; float64 or complex128 as the result is).  It
    equals :func:`trace_full` when the factors carry the quantum dimensions, as the B symbols do."""
    if move is not None:
        mid_codomain, mid_domain, codomain_idcs, domain_idcs, mapping = move
        data = transform_tensor(bb, data, codomain, domain, mid_codomain, mid_domain, codomain_idcs, domain_idcs, mapping)
        codomain, domain = mid_codomain, mid_domain
    for trace in (cod_trace, dom_trace):
        if trace is not None and any(b - a < 2 for a, b in zip(trace.positions, trace.positions[1:])):
            raise ValueError('partial_trace: the traced positions of a side are ascending and do not overlap')
    J = codomain.num_legs
    idcs1 = list(cod_trace.positions if cod_trace is not None else ()) + [J + k for k in (dom_trace.positions if dom_trace is not None else ())]
    idcs2 = [k + 1 for k in idcs1]
    remaining = [k for k in range(J + domain.num_legs) if k not in idcs1 and k not in idcs2]
    scalar = new_codomain.num_legs == 0 and new_domain.num_legs == 0
    where_cod = {tuple(s): k for k, s in enumerate(new_codomain.sectors.tolist())}
    where_dom = {tuple(s): k for k, s in enumerate(new_domain.sectors.tolist())}
    factors = [f for tr in (cod_trace, dom_trace) if tr is not None for _, f in tr.table.values()]
    cplx = any(_is_complex(b) for b in data.blocks) or any(complex(f).imag != 0.0 for f in factors)
    # (new codomain sector, new domain sector) -> the old block that feeds it (None: the scalar of a tensor without that block)
    feeds = {k: None for k in common_sectors(new_codomain, new_domain)} if scalar else {}
    for n, (_, j) in enumerate(data.block_inds.tolist()):
        s = tuple(domain.sectors[j].tolist())
        if s in where_cod and s in where_dom:
            feeds[(where_cod[s], where_dom[s])] = n
    rows = sorted(feeds)
    if not rows:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    outs = bb.empty_many([(new_codomain.block_size(i), new_domain.block_size(j)) for i, j in rows], dtype=np.complex128 if cplx else np.float64)
    outputs = []
    for (i_new, j_new), out in zip(rows, outs):
        tiles = {(xb.tree, yb.tree): (xb, yb, []) for xb in new_codomain.tree_blocks[i_new] for yb in new_domain.tree_blocks[j_new]}
        n = feeds[(i_new, j_new)]
        if n is not None:
            i_old, j_old = data.block_inds[n].tolist()
            dom_side = [(yb, _traced_tree(domain, new_domain, dom_trace, j_old, yb, 'domain')) for yb in domain.tree_blocks[j_old]]
            for xb in codomain.tree_blocks[i_old]:
                hit = _traced_tree(codomain, new_codomain, cod_trace, i_old, xb, 'codomain')
                if hit is None:
                    continue
                nx, f_cod = hit
                for yb, hit2 in dom_side:
                    if hit2 is None:
                        continue
                    ny, f_dom = hit2
                    tile = bb.get_item(data.blocks[n], (slice(xb.start, xb.stop), slice(yb.start, yb.stop)))
                    src = bb.reshape(tile, list(xb.multiplicities) + list(yb.multiplicities))
                    coeff = f_cod * np.conj(f_dom)
                    tiles[(nx.tree, ny.tree)][2].append((src, idcs1, idcs2, remaining, coeff if cplx else float(np.real(coeff))))
        for xb, yb, terms in tiles.values():
            dst = bb.get_item(out, (slice(xb.start, xb.stop), slice(yb.start, yb.stop)))
            outputs.append((bb.reshape(dst, list(xb.multiplicities) + list(yb.multiplicities)), terms))
    bb.tree_trace_many(outputs)
    res = FusionTreeData(np.array(rows, dtype=np.int64), outs)
    return discard_zero_blocks(bb, res, eps) if discard and not scalar else res


# ---------------------------------------------------------------------------------------------------------------------------
# outer

class TreeOuter(NamedTuple):
    """What the symmetry layer knows about the tensor product of the trees of ONE side (codomain or domain), as data:
    ``FusionTree::outer`` (src/symmetries/trees.cpp:1354-1393, F symbols through ``insert_at``), per pair of trees."""
    table: dict        # (a tree key, b tree key) -> [(new tree key, amplitude), ...]; an empty list is allowed, a missing pair is not


def _outer_trees(new_space: TreeSpace, outer_table, seen: dict, xa: TreeBlock, xb: TreeBlock, what: str):
    """[(coupled sector, its index, new TreeBlock, amplitude)] of a pair of trees of one side, checked once per pair"""
    res = seen.get((xa.tree, xb.tree))
    if res is not None:
        return res
    hit = outer_table.table.get((xa.tree, xb.tree))
    if hit is None:
        raise ValueError(f'outer: the {what} table has no entry for the trees {xa.tree!r} and {xb.tree!r}')
    res = []
    for key, amp in hit:
        if not new_space.has_tree(key):
            raise ValueError(f'outer: the new {what} has no tree {key!r}')
        i_new, nb = new_space.tree_block_slice(key)
        if tuple(nb.multiplicities) != tuple(xa.multiplicities) + tuple(xb.multiplicities):
            raise ValueError(f'outer: the multiplicities {tuple(nb.multiplicities)} of a new {what} tree are not those of its factors, '
                             f'{tuple(xa.multiplicities)} followed by {tuple(xb.multiplicities)}')
        res.append((tuple(new_space.sectors[i_new].tolist()), i_new, nb, amp))
    seen[(xa.tree, xb.tree)] = res
    return res


def outer(bb, a: FusionTreeData, a_codomain: TreeSpace, a_domain: TreeSpace, b: FusionTreeData, b_codomain: TreeSpace, b_domain: TreeSpace,
          new_codomain: TreeSpace, new_domain: TreeSpace, cod_outer: TreeOuter, dom_outer: TreeOuter, eps: float = 0.0,
          discard: bool = True) -> FusionTreeData:
    """``FusionTreeBackend::outer`` (fusion_tree_backend.cpp:2609-2667): the tensor product of `a` and `b` on the spaces
    ``new_codomain = a_codomain (x) b_codomain``, ``new_domain = a_domain (x) b_domain`` (:2618-2623).  `cod_outer` /
    `dom_outer`: what ``FusionTree::outer`` says per pair of codomain / domain trees (:class:`TreeOuter`).

    The reference's loops -- tree-block pairs of a (:2626-2630) times tree-block pairs of b (:2631-2635), then the new domain
    trees and the new codomain trees of the same coupled sector (:2642-2650) -- emit one term record per contributing
    (a tree pair, b tree pair) with the coefficient ``conj(u_cod) * v_dom`` (:2653), both tiles read in place, instead of
    outer, permute_axes, combine_legs, get_item, mul, operator+ and set_item.  Every result block that receives at least one
    term gets one output record per (new codomain tree, new domain tree) tile, tiles without a term included (they are
    written as zeros, so the result needs no zero fill); result blocks that receive no term are absent (the reference
    allocates them as zeros and discards them, :2625, :2665).  ONE ``tree_outer_many`` call.

    Order of the terms of a tile: a's blocks ascending, a's codomain trees, a's domain trees, then b's blocks, b's codomain
    trees, b's domain trees (``iter_tree_blocks`` order each); the tiles of a result block are ordered by new codomain tree,
    then new domain tree.  The result is complex if an operand or an amplitude is, sorted by ``block_inds``, and goes through
    :func:`discard_zero_blocks` with `eps` unless ``discard=False``.  A zero-leg operand (a space with one coupled sector,
    one tree without multiplicities, block size 1) is an ordinary 1 x 1 tile."""
    amps = [amp for tb in (cod_outer, dom_outer) for lst in tb.table.values() for _, amp in lst]
    cplx = any(_is_complex(blk) for blk in a.blocks + b.blocks) or any(complex(x).imag != 0.0 for x in amps)
    seen_cod, seen_dom = {}, {}
    b_pairs = []
    for m, (ib, jb) in enumerate(b.block_inds.tolist()):
        for xb in b_codomain.tree_blocks[ib]:
            for yb in b_domain.tree_blocks[jb]:
                b_pairs.append((xb, yb, bb.get_item(b.blocks[m], (slice(xb.start, xb.stop), slice(yb.start, yb.stop)))))
    terms_of: dict = {}      # (i_new, j_new) -> {(new codomain tree, new domain tree): [(A, B, coeff)]}
    for n, (ia, ja) in enumerate(a.block_inds.tolist()):
        for xa in a_codomain.tree_blocks[ia]:
            for ya in a_domain.tree_blocks[ja]:
                A = None
                for xb, yb, B in b_pairs:
                    cods = _outer_trees(new_codomain, cod_outer, seen_cod, xa, xb, 'codomain')
                    doms = _outer_trees(new_domain, dom_outer, seen_dom, ya, yb, 'domain')
                    for sec_d, j_new, ny, v in doms:
                        for sec_c, i_new, nx, u in cods:
                            if sec_c != sec_d:
                                continue                     # (:2649)
                            if A is None:
                                A = bb.get_item(a.blocks[n], (slice(xa.start, xa.stop), slice(ya.start, ya.stop)))
                            coeff = np.conj(u) * v           # (:2653)
                            terms_of.setdefault((i_new, j_new), {}).setdefault((nx.tree, ny.tree), []).append(
                                (A, B, complex(coeff) if cplx else float(np.real(coeff))))
    rows = sorted(terms_of)
    if not rows:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    outs = bb.empty_many([(new_codomain.block_size(i), new_domain.block_size(j)) for i, j in rows], dtype=np.complex128 if cplx else np.float64)
    outputs = []
    for (i_new, j_new), out in zip(rows, outs):
        tiles = terms_of[(i_new, j_new)]
        for nx in new_codomain.tree_blocks[i_new]:
            for ny in new_domain.tree_blocks[j_new]:
                if nx.stop > nx.start and ny.stop > ny.start:
                    dst = bb.get_item(out, (slice(nx.start, nx.stop), slice(ny.start, ny.stop)))
                    outputs.append((dst, tiles.get((nx.tree, ny.tree), [])))
    bb.tree_outer_many(outputs)
    res = FusionTreeData(np.array(rows, dtype=np.int64), outs)
    return discard_zero_blocks(bb, res, eps) if discard else res


# ---------------------------------------------------------------------------------------------------------------------------
# partial_compose

class TreeInsert(NamedTuple):
    """what the symmetry layer knows about inserting b's trees into one leg of the outer trees (FusionTree::insert_at,
    src/symmetries/trees.cpp:1218-1351; the iter_space of fusion_tree_backend.cpp:2697-2747), as data"""
    side: str           # 'codomain' | 'domain': the side of a that is contracted
    leg: int            # leg_idx: position of the inserted leg among the legs of that side, in that side's own order
    outer_trees: dict   # coupled sector (tuple) -> [(outer tree key, b's coupled sector (tuple), m_before, m_after), ...] in iter_tree_blocks order
    table: dict         # (outer tree key, b tree key) -> [(tree key, amplitude), ...]; looked up with b's codomain trees AND b's domain trees


def _inserted_trees(space: TreeSpace, insert: TreeInsert, seen: dict, outer_key, b_key, what: str):
    """[(coupled sector, TreeBlock, amplitude)] of ``outer tree.insert_at(leg, b tree)`` in `space`, checked once per pair"""
    res = seen.get((outer_key, b_key))
    if res is not None:
        return res
    hit = insert.table.get((outer_key, b_key))
    if hit is None:
        raise ValueError(f'partial_compose: the table has no entry for the outer tree {outer_key!r} and the tree {b_key!r} of b')
    res = []
    for key, amp in hit:
        if not space.has_tree(key):
            raise ValueError(f'partial_compose: the {what} has no tree {key!r}')
        i, tb = space.tree_block_slice(key)
        res.append((tuple(space.sectors[i].tolist()), tb, amp))
    seen[(outer_key, b_key)] = res
    return res


def partial_compose(bb, a: FusionTreeData, a_codomain: TreeSpace, a_domain: TreeSpace, b: FusionTreeData, b_codomain: TreeSpace,
                    b_domain: TreeSpace, new_codomain: TreeSpace, new_domain: TreeSpace, insert: TreeInsert, eps: float = 0.0,
                    discard: bool = True) -> FusionTreeData:
    """``FusionTreeBackend::partial_compose`` (fusion_tree_backend.cpp:2670-2880): ALL legs of one side of `b` are contracted
    with a contiguous run of legs of one side of `a` -- b's codomain with legs of a's domain (``insert.side == 'domain'``), or
    b's domain with legs of a's codomain (``'codomain'``) -- without bending and braiding `a` first.  `new_codomain` /
    `new_domain`: the spaces of the result; the side that is not contracted keeps a's space.  `insert`: the outer ("dummy")
    trees of every coupled sector (the ``iter_space`` of :2697-2747, in which the contracted legs are one leg that carries
    b's coupled sectors) and what ``insert_at`` says per (outer tree, tree of b), as data (:class:`TreeInsert`).

    The loops are the reference's.  A block of `a` gives a result block if its coupled sector is in both new spaces
    (:2756-2768).  For every outer tree of that sector (:2771; its b-sector must have a block in `b`, :2775), every codomain
    tree ``xb`` and every domain tree ``yb`` of that block of b (:2787-2794):

    * ``'domain'`` (:2797-2827): old trees (in a's domain) from ``table[(tree, xb)]``, new trees (in the new domain) from
      ``table[(tree, yb)]``, factor ``amp_old * conj(amp_new)`` (:2817); the tree block of b is K x N;
    * ``'codomain'`` (:2828-2857): old trees (in a's codomain) from ``table[(tree, yb)]``, new trees (in the new codomain) from
      ``table[(tree, xb)]``, factor ``conj(amp_old) * amp_new`` (:2847); the tree block of b is N x K.

    The placement of the conjugate is the reference's in both cases; its own TODO at :2687 asks whether the domain case
    should conjugate as the codomain case does, which only a symmetry with complex F symbols can decide.  It is kept as it
    is, not "fixed".

    Instead of get_item, reshape, tdot, permute_axes, reshape, as_scalar, get_item, mul, operator+ and set_item per innermost
    iteration, every result block gets one output record per new tree of the contracted side in tree-block order -- a
    full-height column strip (domain) or a full-width row strip (codomain), strips without a term included (they are written
    as zeros, so the result needs no zero fill) -- and every contributing (outer tree, xb, yb, old tree, new tree) gives one
    term record, in exactly that loop order, with the old strip of a and the tree block of b read in place.  ONE
    ``tree_compose_many`` call for the whole tensor.  The result is complex if `a`, `b` or an amplitude is, sorted by
    ``block_inds``, and goes through :func:`discard_zero_blocks` with `eps` unless ``discard=False`` (:2878).  An empty `a` or
    `b` gives empty data (:2694).

    The kernel behind it is shaped for SMALL contracted extents K and surviving extents N -- the multiplicities of physical
    and MPO legs, a short register loop per result element.  A large K (contracting over a bond leg of dimension chi) is
    still correct but runs at no GEMM rate: bend the legs with :func:`transform_tensor` and use :func:`compose` there."""
    if insert.side not in ('codomain', 'domain'):
        raise ValueError(f"partial_compose: insert.side is 'codomain' or 'domain', not {insert.side!r}")
    if not a.blocks or not b.blocks:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    dom = insert.side == 'domain'
    old_space, new_space = (a_domain, new_domain) if dom else (a_codomain, new_codomain)
    amps = [amp for lst in insert.table.values() for _, amp in lst]
    cplx = any(_is_complex(blk) for blk in a.blocks + b.blocks) or any(complex(x).imag != 0.0 for x in amps)
    where_cod = {tuple(s): k for k, s in enumerate(new_codomain.sectors.tolist())}
    where_dom = {tuple(s): k for k, s in enumerate(new_domain.sectors.tolist())}
    where_b = {tuple(s): k for k, s in enumerate(b_domain.sectors.tolist())}
    seen_old, seen_new = {}, {}
    b_tiles: dict = {}                 # (block of b, xb tree, yb tree) -> view
    rows, shapes, plans = [], [], []
    for n, (i, j) in enumerate(a.block_inds.tolist()):
        coupled = tuple(a_codomain.sectors[i].tolist())
        if coupled not in where_cod or coupled not in where_dom:
            continue                                                     # (:2762)
        i_new, j_new = where_cod[coupled], where_dom[coupled]
        shape = (new_codomain.block_size(i_new), new_domain.block_size(j_new))
        kept, kept_old = (shape[0], a_codomain.block_size(i)) if dom else (shape[1], a_domain.block_size(j))
        if kept != kept_old:
            raise ValueError(f'partial_compose: the result block of the coupled sector {coupled} has {kept} '
                             f'{"rows" if dom else "columns"}, the block of a {kept_old}: the side that is not contracted keeps its space')
        strips = {nb.tree: [nb, None, []] for nb in new_space.tree_blocks[j_new if dom else i_new]}   # tree -> [block, (m0, m2), terms]
        a_strips: dict = {}
        for tree, b_sector, m0, m2 in insert.outer_trees.get(coupled, ()):                            # (:2771)
            jb = where_b.get(tuple(b_sector))
            nb_ = b.block_ind_from_domain_sector(jb) if jb is not None else None
            if nb_ is None:
                raise ValueError(f'partial_compose: b has no block in the coupled sector {tuple(b_sector)} of the outer tree {tree!r}')   # (:2775)
            ib = int(b.block_inds[nb_, 0])
            m0, m2 = int(m0), int(m2)
            for xb in b_codomain.tree_blocks[ib]:                                                     # (:2787)
                for yb in b_domain.tree_blocks[jb]:                                                   # (:2789)
                    kb, sb = (xb, yb) if dom else (yb, xb)          # the tree of b's contracted side, of its surviving side
                    olds = _inserted_trees(old_space, insert, seen_old, tree, kb.tree, f'{insert.side} of a')
                    news = _inserted_trees(new_space, insert, seen_new, tree, sb.tree, f'new {insert.side}')
                    K, N = kb.stop - kb.start, sb.stop - sb.start
                    B = None
                    for sec_old, ob, amp_old in olds:                                                 # (:2799 / :2829)
                        if sec_old != coupled:
                            raise ValueError(f'partial_compose: the old tree {ob.tree!r} lies in the coupled sector {sec_old}, not in {coupled}')
                        if ob.stop - ob.start != m0 * K * m2:
                            raise ValueError(f'partial_compose: the old tree {ob.tree!r} has the size {ob.stop - ob.start}, not m_before * K * '
                                             f'm_after = {m0} * {K} * {m2}')
                        for sec_new, nb, amp_new in news:                                             # (:2807 / :2837)
                            if sec_new != coupled:
                                raise ValueError(f'partial_compose: the new tree {nb.tree!r} lies in the coupled sector {sec_new}, not in {coupled}')
                            if nb.stop - nb.start != m0 * N * m2:
                                raise ValueError(f'partial_compose: the new tree {nb.tree!r} has the size {nb.stop - nb.start}, not m_before * N * '
                                                 f'm_after = {m0} * {N} * {m2}')
                            strip = strips[nb.tree]
                            if strip[1] is None:
                                strip[1] = (m0, m2)
                            elif strip[1] != (m0, m2):
                                raise ValueError(f'partial_compose: the outer trees that feed the new tree {nb.tree!r} differ in (m_before, m_after): '
                                                 f'{strip[1]} and {(m0, m2)}')
                            A = a_strips.get(ob.tree)
                            if A is None:
                                sl = slice(ob.start, ob.stop)
                                A = a_strips[ob.tree] = bb.get_item(a.blocks[n], (slice(None), sl) if dom else (sl, slice(None)))
                            if B is None:
                                B = b_tiles.get((nb_, xb.tree, yb.tree))
                                if B is None:
                                    B = b_tiles[(nb_, xb.tree, yb.tree)] = bb.get_item(
                                        b.blocks[nb_], (slice(xb.start, xb.stop), slice(yb.start, yb.stop)))
                            coeff = amp_old * np.conj(amp_new) if dom else np.conj(amp_old) * amp_new   # (:2817 / :2847)
                            strip[2].append((A, B, complex(coeff) if cplx else float(np.real(coeff))))
        rows.append((i_new, j_new))
        shapes.append(shape)
        plans.append(strips)
    if not rows:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    outs = bb.empty_many(shapes, dtype=np.complex128 if cplx else np.float64)
    outputs = []
    for out, shape, strips in zip(outs, shapes, plans):
        for nb, mm, terms in strips.values():
            if nb.stop > nb.start and shape[0] > 0 and shape[1] > 0:
                sl = slice(nb.start, nb.stop)
                dst = bb.get_item(out, (slice(None), sl) if dom else (sl, slice(None)))
                outputs.append((dst, insert.side, *(mm or (1, 1)), terms))
    bb.tree_compose_many(outputs)
    res = FusionTreeData(np.array(rows, dtype=np.int64), outs).sorted()
    return discard_zero_blocks(bb, res, eps) if discard else res


# ---------------------------------------------------------------------------------------------------------------------------
# dense conversion

class TreeDense(NamedTuple):
    """What the symmetry layer knows about the dense form of ONE side (codomain or domain), as data: the internal basis of
    every flat leg, ``Symmetry::batch_sector_dim`` and ``FusionTree::to_dense_block(bb, nullopt, true)`` per tree."""
    legs: tuple         # per flat leg of this side, in leg order: [(sector key, multiplicity), ...] in the leg's internal basis
                        # order (sorted sectors, each contiguous)
    sector_dims: dict   # sector key -> int dimension
    tensors: dict       # tree -> ndarray of shape (d_a1, ..., d_aJ, d_c), float64 or complex128


MAX_DENSE_LEGS = 6      # flat legs of both sides together (twelve levels (k, m) of the kernel's index space)
_NORM_ROUNDING = 32 * 2.0 ** -53     # relative rounding allowance of the difference of two squared norms (from_dense_block)


def _dense_side(space: TreeSpace, dense: TreeDense, what: str, name: str):
    """-> (per leg {sector key: (start, dimension, multiplicity)}, dimension of every dense axis, per coupled sector the forests
    {uncoupled: [TreeBlock, ...]}, per coupled sector its dimension d_c or None), everything checked"""
    n = space.num_legs
    if len(dense.legs) != n:
        raise ValueError(f'{name}: the {what} has {n} flat legs, its TreeDense lists {len(dense.legs)}')
    where, dims = [], []
    for leg in dense.legs:
        pos, off = {}, 0
        for key, m in leg:
            if key not in dense.sector_dims:
                raise ValueError(f'{name}: no dimension for the sector {key!r} of a {what} leg')
            d = int(dense.sector_dims[key])
            pos[key] = (off, d, int(m))
            off += d * int(m)
        where.append(pos)
        dims.append(off)
    forests, dcs = [], []
    for tbs in space.tree_blocks:
        fs, dc = {}, None
        for tb in tbs:
            if len(tb.uncoupled) != n or len(tb.multiplicities) != n:
                raise ValueError(f'{name}: a {what} tree lacks the uncoupled sector keys of its legs (TreeBlock.uncoupled)')
            if tb.tree not in dense.tensors:
                raise ValueError(f'{name}: the {what} TreeDense has no tensor for the tree {tb.tree!r}')
            for j, (key, m) in enumerate(zip(tb.uncoupled, tb.multiplicities)):
                if key not in where[j] or where[j][key][2] != m:
                    raise ValueError(f'{name}: the multiplicity {m} of leg {j} of the {what} tree {tb.tree!r} is not that of the sector '
                                     f'{key!r} in TreeDense.legs')
            X = np.asarray(dense.tensors[tb.tree])
            want = tuple(where[j][key][1] for j, key in enumerate(tb.uncoupled))
            if X.ndim != n + 1 or X.shape[:-1] != want or (dc is not None and X.shape[-1] != dc):
                raise ValueError(f'{name}: the tensor of the {what} tree {tb.tree!r} has the shape {X.shape}, not {want} and the dimension of '
                                 'its coupled sector')
            dc = X.shape[-1]
            fs.setdefault(tuple(tb.uncoupled), []).append(tb)
        forests.append(fs)
        dcs.append(dc)
    return where, dims, forests, dcs


def _dense_setup(name, codomain: TreeSpace, domain: TreeSpace, cod_dense: TreeDense, dom_dense: TreeDense):
    if codomain.num_legs + domain.num_legs > MAX_DENSE_LEGS:
        raise ValueError(f'{name}: {codomain.num_legs + domain.num_legs} flat legs, at most {MAX_DENSE_LEGS}')
    cod = _dense_side(codomain, cod_dense, 'codomain', name)
    dom = _dense_side(domain, dom_dense, 'domain', name)
    for i, j in common_sectors(codomain, domain):
        if cod[3][i] is not None and dom[3][j] is not None and cod[3][i] != dom[3][j]:
            raise ValueError(f'{name}: the tree tensors of the coupled sector {codomain.sectors[i].tolist()} have the dimension {cod[3][i]} in the '
                             f'codomain and {dom[3][j]} in the domain')
    pairs: dict = {}

    def pair(xa: TreeBlock, yb: TreeBlock):
        """S[k_a..., k_b...] = sum_kc conj(X_alpha[k_a..., kc]) X_beta[k_b..., kc] (:1582-1586), once per pair of trees"""
        S = pairs.get((xa.tree, yb.tree))
        if S is None:
            S = np.ascontiguousarray(np.tensordot(np.conj(cod_dense.tensors[xa.tree]), dom_dense.tensors[yb.tree], ([-1], [-1])))
            pairs[(xa.tree, yb.tree)] = S
        return S

    cplx = any(np.iscomplexobj(X) for td in (cod_dense, dom_dense) for X in td.tensors.values())
    return cod, dom, pair, cplx


def to_dense_block(bb, data: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, cod_dense: TreeDense, dom_dense: TreeDense):
    """``FusionTreeBackend::to_dense_block`` (fusion_tree_backend.cpp:1856-1973 with ``_get_forest_block_contribution``
    :1532-1604) for flat legs, in the internal basis order, for a symmetry that can be dropped: the N-d block with the axes
    (codomain legs..., domain legs reversed) (:1944-1950; the reversal is strides, not a pass).  `cod_dense` / `dom_dense`: what
    the symmetry layer says per leg and per tree (:class:`TreeDense`); the spaces carry ``TreeBlock.uncoupled``.

    Trees of one coupled sector with the same uncoupled sectors form a forest.  On leg j the sector a_j takes d * m positions
    of the dense axis, index ``k * m + mu`` (:1926-1930).  The region of the uncoupled sectors (a..., b...) is
    ``sum_c sum_{alpha, beta} S_{alpha beta} (x) T_{alpha beta}`` over ALL coupled sectors the tuple fuses to (the reference
    accumulates into the same slice, :1937), with S the contracted pair of tree tensors (:1582-1586, built on the host, all of
    a call uploaded as one table) and T the tile of block c at the rows of alpha and the columns of beta.  The reference's
    loops -- blocks (:1881), domain forests (:1885), codomain forests (:1890), trees (:1581-1584) -- emit one region record per
    combination of leg sectors, combinations nothing fuses to included (written as zeros: the regions partition the dense
    tensor, so nothing is zero-filled first), and one term per (block, alpha, beta), ordered by block, then alpha, then beta.
    ONE ``tree_to_dense_many`` call.  complex128 if the data or any tree tensor is complex, else float64."""
    name = 'to_dense_block'
    J, K = codomain.num_legs, domain.num_legs
    (cw, cdims, cfor, _), (dw, ddims, dfor, _), pair, cplx = _dense_setup(name, codomain, domain, cod_dense, dom_dense)
    cplx = cplx or any(_is_complex(blk) for blk in data.blocks)
    terms_of: dict = {}
    for n, (i, j) in enumerate(data.block_inds.tolist()):
        for a_key, alphas in cfor[i].items():
            for b_key, betas in dfor[j].items():
                lst = terms_of.setdefault((a_key, b_key), [])
                for xa in alphas:
                    for yb in betas:
                        lst.append((data.blocks[n], xa.start, yb.start, pair(xa, yb)))
    res = bb.empty_many([tuple(cdims) + tuple(ddims[::-1])], dtype=np.complex128 if cplx else np.float64)[0]
    view = bb.permute_axes(res, list(range(J)) + list(range(J + K - 1, J - 1, -1)))
    regions = []
    for combo in itertools.product(*[list(w.items()) for w in cw + dw]):
        keys = tuple(k for k, _ in combo)
        regions.append((tuple(v[0] for _, v in combo), tuple(v[1] for _, v in combo), tuple(v[2] for _, v in combo), J,
                        terms_of.get((keys[:J], keys[J:]), [])))
    bb.tree_to_dense_many(view, regions)
    return res


def from_dense_block(bb, a, codomain: TreeSpace, domain: TreeSpace, cod_dense: TreeDense, dom_dense: TreeDense, tol: float = 1e-8,
                     discard: bool = True) -> FusionTreeData:
    """``FusionTreeBackend::from_dense_block`` (fusion_tree_backend.cpp:1680-1853 with ``_add_forest_block_entries``
    :1606-1677) for flat legs, in the internal basis order: the projection of the N-d block `a` (axes: codomain legs...,
    domain legs reversed, :1752) onto the symmetric tensors.  Every tile (tree alpha, tree beta) of every common coupled sector
    is ``T[m..., n...] = (1 / d_c) sum_{k_a, k_b} conj(S_{alpha beta}[k_a..., k_b...]) a_region[(k_a, m), (k_b, n)]`` (:1656-1662,
    divided after the sum) -- one output record per tile, read from `a` in place; ONE ``tree_from_dense_many`` call, no zero
    fill (the tiles partition the blocks).  One block per common coupled sector; with `discard` those of magnitude <= 1e-14
    are dropped (:1827-1829, :func:`discard_zero_blocks`).  With ``tol != 0``: ValueError if
    ``|a|^2 - sum_c d_c |block_c|^2 > tol^2 |a|^2`` (:1834-1838; the weighted :func:`norm` and the block backend's norm).  The two
    squared norms are float64 reductions in different orders, each within a few 2^-53 relative, and the default ``tol^2 = 1e-16``
    is 2^-53 itself: the comparison allows ``_NORM_ROUNDING = 32 * 2^-53`` on top of ``tol^2``, without which a block that is
    symmetric to the last bit raises whenever the two reductions round differently."""
    name = 'from_dense_block'
    J, K = codomain.num_legs, domain.num_legs
    (cw, cdims, _, cdc), (dw, ddims, _, ddc), pair, cplx = _dense_setup(name, codomain, domain, cod_dense, dom_dense)
    if tuple(a.shape) != tuple(cdims) + tuple(ddims[::-1]):
        raise ValueError(f'{name}: a dense block of shape {tuple(a.shape)} for legs of the dimensions {tuple(cdims) + tuple(ddims[::-1])}')
    cplx = cplx or _is_complex(a)
    view = bb.permute_axes(a, list(range(J)) + list(range(J + K - 1, J - 1, -1)))
    rows = common_sectors(codomain, domain)
    if not rows:
        res = FusionTreeData(np.zeros((0, 2), np.int64), [])
    else:
        outs = bb.empty_many([(codomain.block_size(i), domain.block_size(j)) for i, j in rows], dtype=np.complex128 if cplx else np.float64)
        outputs = []
        for (i, j), out in zip(rows, outs):
            for xa in codomain.tree_blocks[i]:
                for yb in domain.tree_blocks[j]:
                    if xa.stop == xa.start or yb.stop == yb.start:
                        continue
                    at = [cw[l][key] for l, key in enumerate(xa.uncoupled)] + [dw[l][key] for l, key in enumerate(yb.uncoupled)]
                    dst = bb.get_item(out, (slice(xa.start, xa.stop), slice(yb.start, yb.stop)))
                    outputs.append((dst, float(cdc[i]), tuple(v[1] for v in at), tuple(v[2] for v in at), J,
                                    [(view, tuple(v[0] for v in at), pair(xa, yb))]))
        bb.tree_from_dense_many(outputs)
        res = FusionTreeData(np.array(rows, dtype=np.int64), outs)
    if tol != 0.0:
        a_norm_sq = float(bb.norm(a)) ** 2
        if a_norm_sq - norm(bb, res, codomain) ** 2 > (tol * tol + _NORM_ROUNDING) * a_norm_sq:
            raise ValueError(f'{name}: the block is not symmetric up to tolerance')
    return discard_zero_blocks(bb, res, 1e-14) if discard else res


# ---------------------------------------------------------------------------------------------------------------------------
# constructors: from_grid, from_tree_pairs, eye

MAX_PLACE_LEGS = 6      # flat legs of one side of a from_tree_pairs block (the levels of one side of a window's source)


class _Window(NamedTuple):
    """one window of a result block: rows ``r0 : r0 + h`` and columns ``c0 : c0 + wn`` of every one of the `nq` runs of the tile
    ``(x0 : x1, y0 : y1)`` of block `n`, fed by ``coeff * src`` (a view whose first `n_row` axes are the rows) or by zeros"""
    n: int
    x0: int
    x1: int
    y0: int
    y1: int
    nq: int
    r0: int
    h: int
    c0: int
    wn: int
    src: object
    n_row: int
    coeff: object


def _place_windows(bb, shapes, cplx, windows):
    """the result blocks of the given shapes with every window written: ONE ``tree_place_many`` call into blocks that are not
    zero-filled (the windows of a block partition it); a backend without that call takes ``zeros_many`` and, per window with a
    source, get_item / reshape / set_item as the reference does"""
    dtype = np.complex128 if cplx else np.float64
    windows = [w for w in windows if w.h > 0 and w.nq > 0 and w.wn > 0]
    fused = hasattr(bb, 'tree_place_many')
    outs = bb.empty_many(shapes, dtype=dtype) if fused else bb.zeros_many(shapes, dtype=dtype)
    if fused:
        tiles, records = {}, []
        for w in windows:
            t3 = tiles.get((w.n, w.x0, w.y0))
            if t3 is None:
                tile = bb.get_item(outs[w.n], (slice(w.x0, w.x1), slice(w.y0, w.y1)))
                t3 = tiles[(w.n, w.x0, w.y0)] = bb.reshape(tile, (w.x1 - w.x0, w.nq, (w.y1 - w.y0) // w.nq))
            dst = bb.get_item(t3, (slice(w.r0, w.r0 + w.h), slice(None), slice(w.c0, w.c0 + w.wn)))
            records.append((dst, w.src, w.n_row, w.coeff))
        bb.tree_place_many(records)
        return outs
    for w in windows:
        if w.src is None:
            continue
        value = bb.reshape(w.src, (w.h, w.nq, w.wn))
        if w.coeff != 1:
            value = bb.mul(w.coeff, value)
        key = (slice(w.x0, w.x1), slice(w.y0, w.y1))
        t3 = bb.reshape(bb.get_item(outs[w.n], key), (w.x1 - w.x0, w.nq, (w.y1 - w.y0) // w.nq))
        bb.set_item(t3, (slice(w.r0, w.r0 + w.h), slice(None), slice(w.c0, w.c0 + w.wn)), value)
        bb.set_item(outs[w.n], key, bb.reshape(t3, (w.x1 - w.x0, w.y1 - w.y0)))
    return outs


def _grid_slices(table, key, n, total, what):
    """the cumulative multiplicity table of the sector `key` of a stacked leg: n + 1 ascending entries from 0 to `total`"""
    try:
        s = [int(v) for v in table[key]]
    except (KeyError, IndexError, TypeError):
        raise ValueError(f'from_grid: {what} has no entry for the sector {key!r}') from None
    if len(s) != n + 1 or s[0] != 0 or any(b < a for a, b in zip(s, s[1:])):
        raise ValueError(f'from_grid: {what}[{key!r}] = {s} is no ascending table of {n + 1} entries that starts at 0')
    if s[-1] != total:
        raise ValueError(f'from_grid: {what}[{key!r}] ends at {s[-1]}, the multiplicity of that sector in the new space is {total}')
    return s


def _zero_windows(zero):
    """maximal rectangles (i0, i1, j0, j1) of a boolean cell matrix: runs of zero cells along every row, equal runs of
    consecutive rows merged"""
    runs = []
    for row in zero:
        rr, j = [], 0
        while j < len(row):
            if row[j]:
                j0 = j
                while j < len(row) and row[j]:
                    j += 1
                rr.append((j0, j))
            else:
                j += 1
        runs.append(rr)
    out, open_ = [], {}          # open_: (j0, j1) -> first row of the rectangle that still grows
    for i, rr in enumerate(runs + [[]]):
        for key in [k for k in open_ if k not in rr]:
            out.append((open_.pop(key), i, key[0], key[1]))
        for key in rr:
            open_.setdefault(key, i)
    return sorted(out)


def from_grid(bb, grid, new_codomain: TreeSpace, new_domain: TreeSpace, left_slices, right_slices, factors=None, eps: float = 0.0,
              discard: bool = True) -> FusionTreeData:
    """``FusionTreeBackend::from_grid`` (fusion_tree_backend.cpp:3375-3518, under ``tensor_from_grid``): the tensor whose
    ``codomain[0]`` is the direct sum of that leg over the rows of `grid` and whose ``domain[-1]`` the direct sum over its
    columns; every other leg is the same in all entries.  `grid`: a list of rows of :class:`TreeTensor` or None.
    `new_codomain` / `new_domain` and the cumulative multiplicity tables come from the symmetry layer as data:
    ``left_slices[a][i] : left_slices[a][i + 1]`` are the positions row i takes inside the multiplicity of sector ``a`` of the
    stacked codomain leg, ``right_slices[b][j] : right_slices[b][j + 1]`` those of column j inside sector ``b`` of the stacked
    domain leg; ``a`` / ``b`` is the first / last entry of ``TreeBlock.uncoupled``.  `factors`: a coefficient per cell
    (``factors[i][j]``, default 1; that of an empty cell is not read).

    A tree of an entry is found in the new space by its ``tree`` key: the trees of a forest depend on the uncoupled sectors,
    the coupled sector and the dualities, not on the multiplicities, so an entry's tree IS a tree of the new space (the
    reference matches them by their position inside the forest, :3424-3433).

    For every coupled sector common to the new spaces and every (new codomain tree x, new domain tree y) the tile is
    partitioned into cells (i, j) of positive width.  With Rc the product of x's multiplicities after the first, Rd that of
    y's before the last and n' y's last multiplicity, cell (i, j) is the window of the rows ``left_slices[a][i] * Rc`` onward,
    ``m0 * Rc`` of them, and of Rd runs of ``right_slices[b][j + 1] - right_slices[b][j]`` columns from column
    ``right_slices[b][j]`` on, one run every n' columns -- the six-axis reshape of :3456-3506 per tree.  A cell whose entry
    holds that block is a copy record of the entry's own tile, read in place through its strides (a :func:`dagger` view as it
    stands) under the cell's factor; every other cell is a record of zeros, adjacent ones merged.  ONE ``tree_place_many``
    call: every element of the result is written once, nothing is zero-filled first, a float64 entry beside complex ones is
    read as it stands.

    Result blocks that receive no copy record are absent (the reference allocates all of them as zeros and discards them,
    :3391, :3516); the others go through :func:`discard_zero_blocks` with `eps` unless ``discard=False``.  Sorted by
    ``block_inds``; complex if an entry or a factor is.  ValueError: an empty or ragged grid, a row or column without an entry,
    a slice table without a sector's key or at odds with the multiplicities, an entry whose tree is missing from the new space
    or differs from it in a multiplicity other than the stacked one."""
    grid = [list(row) for row in grid]
    if not grid or not grid[0]:
        raise ValueError('from_grid: an empty grid')
    nr, nc = len(grid), len(grid[0])
    if any(len(row) != nc for row in grid):
        raise ValueError('from_grid: the rows of the grid differ in their length')
    for i, row in enumerate(grid):
        if all(op is None for op in row):
            raise ValueError(f'from_grid: row {i} of the grid has no entry')
    for j in range(nc):
        if all(row[j] is None for row in grid):
            raise ValueError(f'from_grid: column {j} of the grid has no entry')
    if factors is not None:
        factors = [list(row) for row in factors]
        if len(factors) != nr or any(len(row) != nc for row in factors):
            raise ValueError(f'from_grid: factors for a grid of {nr} x {nc} cells are {nr} rows of {nc} numbers')
    if new_codomain.num_legs < 1 or new_domain.num_legs < 1:
        raise ValueError('from_grid: the rows stack on codomain[0] and the columns on domain[-1]: both sides need a leg')
    coeff_of = lambda i, j: 1.0 if factors is None else factors[i][j]                    # noqa: E731
    entries = [(i, j, op) for i, row in enumerate(grid) for j, op in enumerate(row) if op is not None]
    cplx = any(_is_complex(b) for _, _, op in entries for b in op.blocks) or any(complex(coeff_of(i, j)).imag != 0.0 for i, j, _ in entries)
    where_cod = {tuple(s): k for k, s in enumerate(new_codomain.sectors.tolist())}
    where_dom = {tuple(s): k for k, s in enumerate(new_domain.sectors.tolist())}
    J, K = new_codomain.num_legs, new_domain.num_legs
    feeds: dict = {}         # (i_new, j_new) -> {(x tree, y tree): {(i, j): (block, xe, ye)}}
    for i, j, op in entries:
        for n, (ic, jd) in enumerate(op.block_inds.tolist()):
            coupled = tuple(op.domain.sectors[jd].tolist())
            if coupled not in where_cod or coupled not in where_dom:
                continue                                                     # (:3411-3413)
            rc = (where_cod[coupled], where_dom[coupled])
            new_of = []
            for tbs, space, legs, stacked, table, pos, what in ((op.codomain.tree_blocks[ic], new_codomain, J, 0, left_slices, i, 'codomain'),
                                                                 (op.domain.tree_blocks[jd], new_domain, K, -1, right_slices, j, 'domain')):
                side = []
                for te in tbs:
                    if len(te.uncoupled) != legs or len(te.multiplicities) != legs:
                        raise ValueError(f'from_grid: a {what} tree of entry ({i}, {j}) lacks the uncoupled sector keys or the multiplicities of '
                                         f'its {legs} legs (TreeBlock.uncoupled, TreeBlock.multiplicities)')
                    if not space.has_tree(te.tree):
                        raise ValueError(f'from_grid: the new {what} has no tree {te.tree!r} of entry ({i}, {j})')
                    k_new, tn = space.tree_block_slice(te.tree)
                    if k_new != rc[0 if what == 'codomain' else 1]:
                        raise ValueError(f'from_grid: the tree {te.tree!r} of entry ({i}, {j}) lies in another coupled sector of the new {what}')
                    me, mn = list(te.multiplicities), list(tn.multiplicities)
                    del me[stacked], mn[stacked]
                    if me != mn:
                        raise ValueError(f'from_grid: the multiplicities {tuple(te.multiplicities)} of the {what} tree {te.tree!r} of entry '
                                         f'({i}, {j}) differ from {tuple(tn.multiplicities)} in a leg other than the stacked one')
                    s = _grid_slices(table, te.uncoupled[stacked], nr if what == 'codomain' else nc, tn.multiplicities[stacked],
                                     'left_slices' if what == 'codomain' else 'right_slices')
                    if s[pos + 1] - s[pos] != te.multiplicities[stacked]:
                        raise ValueError(f'from_grid: entry ({i}, {j}) has the multiplicity {te.multiplicities[stacked]} in the sector '
                                         f'{te.uncoupled[stacked]!r} of its stacked {what} leg, its slice is {s[pos]}:{s[pos + 1]}')
                    side.append((te, tn))
                new_of.append(side)
            for xe, xn in new_of[0]:
                for ye, yn in new_of[1]:
                    if xe.stop > xe.start and ye.stop > ye.start:
                        feeds.setdefault(rc, {}).setdefault((xn.tree, yn.tree), {})[(i, j)] = (op.blocks[n], xe, ye)
    rows = sorted(feeds)
    if not rows:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    windows = []
    for n, (i_new, j_new) in enumerate(rows):
        tiles = feeds[(i_new, j_new)]
        for x in new_codomain.tree_blocks[i_new]:
            for y in new_domain.tree_blocks[j_new]:
                if x.stop == x.start or y.stop == y.start:
                    continue
                if len(x.uncoupled) != J or len(x.multiplicities) != J or len(y.uncoupled) != K or len(y.multiplicities) != K:
                    raise ValueError('from_grid: a tree of the new spaces lacks the uncoupled sector keys or the multiplicities of its legs '
                                     '(TreeBlock.uncoupled, TreeBlock.multiplicities)')
                L = _grid_slices(left_slices, x.uncoupled[0], nr, x.multiplicities[0], 'left_slices')
                R = _grid_slices(right_slices, y.uncoupled[-1], nc, y.multiplicities[-1], 'right_slices')
                Rc, Rd = int(np.prod(x.multiplicities[1:], dtype=np.int64)), int(np.prod(y.multiplicities[:-1], dtype=np.int64))
                ri = [i for i in range(nr) if L[i + 1] > L[i]]
                cj = [j for j in range(nc) if R[j + 1] > R[j]]
                cells = tiles.get((x.tree, y.tree), {})
                for i in ri:
                    for j in cj:
                        hit = cells.get((i, j))
                        if hit is not None:
                            blk, xe, ye = hit
                            src = bb.get_item(blk, (slice(xe.start, xe.stop), slice(ye.start, ye.stop)))
                            c = coeff_of(i, j)
                            windows.append(_Window(n, x.start, x.stop, y.start, y.stop, Rd, L[i] * Rc, (L[i + 1] - L[i]) * Rc, R[j], R[j + 1] - R[j],
                                                   src, 1, complex(c) if cplx else float(np.real(c))))
                for a0, a1, b0, b1 in _zero_windows([[(i, j) not in cells for j in cj] for i in ri]):
                    # (rows and columns of positive width are adjacent in the tile: what lies between them has the width 0)
                    r0, r1, c0, c1 = L[ri[a0]], L[ri[a1 - 1] + 1], R[cj[b0]], R[cj[b1 - 1] + 1]
                    windows.append(_Window(n, x.start, x.stop, y.start, y.stop, Rd, r0 * Rc, (r1 - r0) * Rc, c0, c1 - c0, None, 0, 0.0))
    shapes = [(new_codomain.block_size(i), new_domain.block_size(j)) for i, j in rows]
    outs = _place_windows(bb, shapes, cplx, windows)
    res = FusionTreeData(np.array(rows, dtype=np.int64), outs)
    return discard_zero_blocks(bb, res, eps) if discard else res


def from_tree_pairs(bb, trees: dict, codomain: TreeSpace, domain: TreeSpace, dtype=None) -> FusionTreeData:
    """``FusionTreeBackend::from_tree_pairs`` (fusion_tree_backend.cpp:3186-3263).  `trees`: ``{(codomain tree key, domain tree
    key): block}`` with a block of the shape ``(m_1 .. m_J, n_K .. n_1)`` -- the multiplicities of the codomain tree followed by
    those of the domain tree reversed.  Every block is ONE copy record into its tile: the row levels are ``m_1 .. m_J`` with
    the block's own strides, the column levels ``n_1 .. n_K`` with the strides of its axes ``J + K - 1 .. J``; the permutation and
    the reshape of :3226-3233 are never made, a block that is a view is read in place.  Tiles without an entry inside a coupled
    block that holds at least one are records of zeros; coupled sectors without an entry are absent (:3242).  ONE
    ``tree_place_many`` call.  complex128 if `dtype` or a block is complex.  ValueError: a key that no tile takes (the
    reference's "uncovered tree pair", :3247-3249), a block of the wrong shape, more than six legs on a side, a complex block
    under a real `dtype`."""
    J, K = codomain.num_legs, domain.num_legs
    if J > MAX_PLACE_LEGS or K > MAX_PLACE_LEGS:
        raise ValueError(f'from_tree_pairs: {J} codomain legs and {K} domain legs, at most {MAX_PLACE_LEGS} on a side')
    data_cplx = any(_is_complex(b) for b in trees.values())
    cplx = data_cplx if dtype is None else np.dtype(dtype).kind == 'c'
    if data_cplx and not cplx:
        raise ValueError(f'from_tree_pairs: a complex block under the dtype {np.dtype(dtype)}')
    perm = list(range(J)) + list(range(J + K - 1, J - 1, -1))
    rows, shapes, windows, covered = [], [], [], set()
    for i, j in common_sectors(codomain, domain):
        tiles = []
        for xb in codomain.tree_blocks[i]:
            for yb in domain.tree_blocks[j]:
                blk = trees.get((xb.tree, yb.tree))
                if blk is not None:
                    want = tuple(xb.multiplicities) + tuple(yb.multiplicities)[::-1]
                    if len(xb.multiplicities) != J or len(yb.multiplicities) != K or tuple(blk.shape) != want:
                        raise ValueError(f'from_tree_pairs: the block of the trees {xb.tree!r} and {yb.tree!r} has the shape {tuple(blk.shape)}, '
                                         f'not {want}')
                    covered.add((xb.tree, yb.tree))
                tiles.append((xb, yb, blk))
        if all(blk is None for _, _, blk in tiles):
            continue                                                         # (is_zero_block, :3242)
        for xb, yb, blk in tiles:
            src = bb.permute_axes(blk, perm) if blk is not None else None
            windows.append(_Window(len(rows), xb.start, xb.stop, yb.start, yb.stop, 1, 0, xb.stop - xb.start, 0, yb.stop - yb.start,
                                   src, J if blk is not None else 0, 1.0))
        rows.append((i, j))
        shapes.append((codomain.block_size(i), domain.block_size(j)))
    missing = [k for k in trees if k not in covered]
    if missing:
        raise ValueError(f'from_tree_pairs: uncovered tree pair {missing[0]!r}: no tile of a common coupled sector takes it')
    if not rows:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    return FusionTreeData(np.array(rows, dtype=np.int64), _place_windows(bb, shapes, cplx, windows))


def eye(bb, space: TreeSpace, dtype=None) -> FusionTreeData:
    """``FusionTreeBackend::eye_data`` (fusion_tree_backend.cpp:1180-1192): the identity block of every coupled sector of
    `space`, ``block_inds`` (i, i).  The identity has the same matrix elements in every orthonormal basis, so the trees play no
    role.  What most cells of an MPO grid hold."""
    n = space.num_sectors
    return FusionTreeData(np.array([(i, i) for i in range(n)], dtype=np.int64).reshape(n, 2),
                          [bb.eye_matrix(space.block_size(i), dtype=dtype) for i in range(n)])


# ---------------------------------------------------------------------------------------------------------------------------
# vector-space operations

def _match(a_keys, b_keys):
    """(n_a or None, n_b or None) over the union of two ascending duplicate-free key arrays, ascending
    (``iter_common_noncommon_sorted_1d``)"""
    ia = {int(k): n for n, k in enumerate(a_keys)}
    ib = {int(k): n for n, k in enumerate(b_keys)}
    return [(ia.get(k), ib.get(k)) for k in sorted(set(ia) | set(ib))]


def inner(bb, a: FusionTreeData, b: FusionTreeData, codomain: TreeSpace, do_dagger: bool = False):
    """fusion_tree_backend.cpp:1238-1259: sum over the common coupled sectors of qdim * inner(block_a, block_b, do_dagger) --
    ``do_dagger``: <a|b> with b on the spaces of a; else trace(a b) with b's domain on a's codomain.  ONE weighted
    reduction.  `codomain`: a's."""
    col = 0 if do_dagger else 1
    pairs = [(n, m) for n, m in _match(a.block_inds[:, 0], np.sort(b.block_inds[:, col])) if n is not None and m is not None]
    if not pairs:
        return 0.0
    where = {int(k): m for m, k in enumerate(b.block_inds[:, col])}
    xs = [a.blocks[n] for n, _ in pairs]
    ys = [b.blocks[where[int(a.block_inds[n, 0])]] for n, _ in pairs]
    return bb.inner_weighted_many(xs, ys, [codomain.qdims[a.block_inds[n, 0]] for n, _ in pairs], do_dagger=do_dagger)


def trace_full(bb, a: FusionTreeData, codomain: TreeSpace):
    """fusion_tree_backend.cpp:1261-1278: sum_n qdim(coupled_n) trace(block_n), ONE weighted reduction over the diagonals"""
    if not a.blocks:
        return 0.0
    return bb.trace_weighted_many(a.blocks, codomain.qdims[a.block_inds[:, 0]])


def mul(bb, scalar, a: FusionTreeData) -> FusionTreeData:
    """fusion_tree_backend.cpp:1298-1314: a zero scalar gives the tensor without blocks"""
    if scalar == 0 or not a.blocks:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    return FusionTreeData(a.block_inds.copy(), bb.mul_many(scalar, a.blocks))


def linear_combination(bb, a, v: FusionTreeData, b, w: FusionTreeData) -> FusionTreeData:
    """fusion_tree_backend.cpp:1316-1360: a v + b w; a coupled sector only one of them holds gets a * block or b * block
    (:1335-1356).  One batched call for the common blocks and one for each of the two one-sided lists."""
    pairs = _match(v.block_inds[:, 0], w.block_inds[:, 0])
    both = [(i, j) for i, j in pairs if i is not None and j is not None]
    only_v = [i for i, j in pairs if j is None]
    only_w = [j for i, j in pairs if i is None]
    cplx = any(np.dtype(getattr(x, 'dtype', float)).kind == 'c' for x in v.blocks + w.blocks)
    one = complex(1.0) if cplx else 1.0      # (the common dtype of :1324-1332: a one-sided block of a mixed pair is promoted too)
    out = {}
    if both:
        res = bb.linear_combination_many(a, [v.blocks[i] for i, _ in both], b, [w.blocks[j] for _, j in both])
        out.update({('v', i): r for (i, _), r in zip(both, res)})
    if only_v:
        out.update({('v', i): r for i, r in zip(only_v, bb.mul_many(a * one, [v.blocks[i] for i in only_v]))})
    if only_w:
        out.update({('w', j): r for j, r in zip(only_w, bb.mul_many(b * one, [w.blocks[j] for j in only_w]))})
    rows, blocks = [], []
    for i, j in pairs:
        rows.append(v.block_inds[i] if i is not None else w.block_inds[j])
        blocks.append(out[('v', i)] if i is not None else out[('w', j)])
    return FusionTreeData(np.array(rows, dtype=np.int64).reshape(len(rows), 2), blocks)


def dagger(bb, a: FusionTreeData) -> FusionTreeData:
    """fusion_tree_backend.cpp:717-729: the columns of ``block_inds`` swap (codomain and domain have swapped), the rows are
    sorted again, every block is the conjugate of its transposed view: a real block stays a view (the kernels read strides), the
    complex blocks of the tensor are conjugated by ONE batched copy"""
    views = [bb.permute_axes(blk, [1, 0]) for blk in a.blocks]
    cplx = [n for n, blk in enumerate(a.blocks) if _is_complex(blk)]
    if cplx:
        outs = bb.empty_many([tuple(views[n].shape) for n in cplx], dtype=np.complex128)
        bb.copy_many([(o, views[n]) for o, n in zip(outs, cplx)], conj=True)
        for o, n in zip(outs, cplx):
            views[n] = o
    return FusionTreeData(a.block_inds[:, ::-1].copy(), views).sorted()


def almost_equal(bb, a: FusionTreeData, b: FusionTreeData, rtol: float = 1e-5, atol: float = 1e-8) -> bool:
    """fusion_tree_backend.cpp:560-590: blocks only one tensor holds must vanish within atol, common ones be allclose.  As in
    the reference this is a reduction and a host wait per coupled sector, ending at the first sector that differs: a
    comparison for tests and convergence checks, not part of an update step."""
    for i, j in _match(a.block_inds[:, 0], b.block_inds[:, 0]):
        if j is None:
            ok = bb.max_abs(a.blocks[i]) <= atol
        elif i is None:
            ok = bb.max_abs(b.blocks[j]) <= atol
        else:
            ok = bb.allclose(a.blocks[i], b.blocks[j], rtol, atol)
        if not ok:
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------------
# axis operations on tree blocks

class TreeAxisRecord(NamedTuple):
    """one tree block of one coupled block on one side, as ``tree_axis_many`` reads it: tree position
    ``t = (o * A + a) * inner + i`` counted from ``src_start`` / ``dst_start``"""
    src: object        # coupled block (2-D) or diagonal block (1-D), read in place
    dst: object        # result block, written in place
    side: int          # 0: tree blocks are row ranges (codomain), 1: column ranges (domain)
    src_start: int
    dst_start: int
    outer: int
    A: int             # multiplicity of the acted leg in the source
    A_dst: int         # ... in the destination
    inner: int
    table: object      # scale: 1-D block of A factors; gather / scatter: kept positions (host int64 array or DeviceIndex)


@dataclass
class TreeMask:
    """A mask on one leg: per sector of the large leg (a hashable key, as in ``TreeBlock.uncoupled``) its multiplicity and the
    ascending kept positions -- a host int64 array, a ``DeviceIndex`` (the table ``truncate_select`` left on the device) or
    None (nothing kept; also the meaning of a sector the mask does not list)."""
    sectors: list
    large_mults: list
    keep: list
    _pos: dict = field(default_factory=dict, repr=False)

    def __post_init__(self):
        self._pos = {k: n for n, k in enumerate(self.sectors)}
        self.keep = [None if t is None else (t if hasattr(t, 'ptr') else np.asarray(t, dtype=np.int64)) for t in self.keep]

    def table(self, key):
        n = self._pos.get(key)
        return None if n is None else self.keep[n]

    def small(self, key) -> int:
        t = self.table(key)
        return 0 if t is None else (t.n if hasattr(t, 'ptr') else len(t))

    def large(self, key) -> int:
        n = self._pos.get(key)
        return 0 if n is None else int(self.large_mults[n])

    @classmethod
    def from_truncation(cls, mask_blocks, mask_block_inds, leg_space: TreeSpace, tables=None) -> 'TreeMask':
        """the mask :func:`truncate_singular_values` returned (boolean host vectors, rows (small index, large index j)) on
        the one-leg space it was computed for; `tables`: ``{j: DeviceIndex}`` to use instead of the host positions"""
        keys = leg_keys(leg_space)
        keep = [None] * len(keys)
        for blk, (_, j) in zip(mask_blocks, np.asarray(mask_block_inds).reshape(-1, 2).tolist()):
            keep[j] = tables[j] if tables is not None else np.flatnonzero(blk)
        return cls(keys, [int(m) for m in leg_space.multiplicities], keep)


def leg_keys(space: TreeSpace) -> list:
    """sector key of every coupled sector of a one-leg space: the ``uncoupled`` key of its tree, else the sector itself"""
    keys = []
    for i, tbs in enumerate(space.tree_blocks):
        if len(tbs) != 1 or len(tbs[0].multiplicities) != 1:
            raise ValueError('a one-leg space has one tree with one multiplicity per sector')
        keys.append(tbs[0].uncoupled[0] if tbs[0].uncoupled else tuple(space.sectors[i].tolist()))
    return keys


def _parse_leg(codomain: TreeSpace, domain: TreeSpace, leg: int):
    """(side, index within the side) of a leg numbered as in :func:`transform_tensor`: the codomain legs, then the domain
    legs counted from the end"""
    J, N = codomain.num_legs, codomain.num_legs + domain.num_legs
    if not 0 <= leg < N:
        raise ValueError(f'leg {leg} outside [0, {N})')
    return (0, leg) if leg < J else (1, N - 1 - leg)


def _split(tb: TreeBlock, idx: int):
    if len(tb.uncoupled) != len(tb.multiplicities) or idx >= len(tb.multiplicities):
        raise ValueError('this operation needs the uncoupled sector keys of every tree (TreeBlock.uncoupled)')
    m = tb.multiplicities
    return int(np.prod(m[:idx], dtype=np.int64)), int(m[idx]), int(np.prod(m[idx + 1:], dtype=np.int64)), tb.uncoupled[idx]


def _is_complex(blk) -> bool:
    return np.dtype(getattr(blk, 'dtype', float)).kind == 'c'


def scale_axis(bb, data: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, diag: FusionTreeData, diag_space: TreeSpace,
               leg: int) -> FusionTreeData:
    """fusion_tree_backend.cpp:3521-3644: every tree block is multiplied along `leg` (numbered as in :func:`transform_tensor`)
    with the diagonal block of its uncoupled sector there.  `diag`: 1-D blocks on the one-leg `diag_space`.  Tree blocks
    whose sector has no diagonal block give zeros; a coupled block none of whose trees has one is absent (:3596-3605).  The
    one-leg side (:3544-3568) is the general case with ``outer = inner = 1``.  ONE launch."""
    side, idx = _parse_leg(codomain, domain, leg)
    space = domain if side else codomain
    keys = leg_keys(diag_space)
    f_of = {keys[int(j)]: diag.blocks[n] for n, j in enumerate(diag.block_inds[:, 0])}
    cplx = any(_is_complex(b) for b in data.blocks) or any(_is_complex(b) for b in diag.blocks)
    plan, rows, shapes = [], [], []
    for n, (i, j) in enumerate(data.block_inds.tolist()):
        recs = []
        for tb in space.tree_blocks[j if side else i]:
            outer, A, inner, key = _split(tb, idx)
            f = f_of.get(key)
            if f is not None and tb.stop > tb.start:
                recs.append((tb.start, outer, A, inner, f))
        if not recs:
            continue
        covered = sum(o * A * i_ for _, o, A, i_, _ in recs) == space.block_size(j if side else i)
        plan.append((n, recs, covered))
        rows.append((i, j))
        shapes.append(tuple(data.blocks[n].shape))
    if not plan:
        return FusionTreeData(np.zeros((0, 2), np.int64), [])
    outs = bb.empty_many(shapes, dtype=np.complex128 if cplx else np.float64)
    records = [TreeAxisRecord(data.blocks[n], out, side, start, start, outer, A, A, inner, f)
               for (n, recs, _), out in zip(plan, outs) for start, outer, A, inner, f in recs]
    bb.tree_axis_many(records, 'scale', fill=[out for (_, _, covered), out in zip(plan, outs) if not covered])
    return FusionTreeData(np.array(rows, dtype=np.int64), outs)


def _masked_space(space: TreeSpace, idx: int, mask: TreeMask, large_leg: bool) -> TreeSpace:
    """the space with the multiplicity of leg `idx` replaced by the mask's small (`large_leg`) or large one: the same trees
    in the same order, empty trees and then empty coupled sectors dropped"""
    keep, blocks = [], []
    for i, tbs in enumerate(space.tree_blocks):
        off, new = 0, []
        for tb in tbs:
            _, _, _, key = _split(tb, idx)
            m = list(tb.multiplicities)
            m[idx] = mask.small(key) if large_leg else mask.large(key)
            sz = int(np.prod(m, dtype=np.int64))
            if sz:
                new.append(TreeBlock(tb.tree, off, off + sz, tuple(m), tb.uncoupled))
                off += sz
        if new:
            keep.append(i)
            blocks.append(new)
    return TreeSpace(space.sectors[keep], space.qdims[keep], blocks, space.num_legs)


def mask_contract(bb, data: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, mask: TreeMask, leg: int, large_leg: bool = True,
                  target: TreeSpace = None, eps: float = 0.0, discard: bool = True):
    """fusion_tree_backend.cpp:2372-2500: project `leg` (numbered as in :func:`transform_tensor`) with the mask
    (``large_leg=True``: the leg is the mask's large leg, ``apply_mask`` per tree block) or embed it (``False``: the leg is the
    small leg, ``enlarge_leg``).  Returns (data, new codomain, new domain).  `target`: the new space of that side; if not
    given it is derived (:func:`_masked_space`, and ``block_inds`` re-indexed, :2424-2439).  ONE launch; the result goes
    through :func:`discard_zero_blocks` with `eps` (the reference's ``fusion_tree_eps``) unless ``discard=False`` -- the switch
    :func:`truncated_svd` uses, whose isometries have no zero blocks and which must not wait for the host per block.  Defined per tree block (the module docstring
    names the difference to :2471)."""
    side, idx = _parse_leg(codomain, domain, leg)
    space = domain if side else codomain
    new_space = target if target is not None else _masked_space(space, idx, mask, large_leg)
    where = {tuple(s): k for k, s in enumerate(new_space.sectors.tolist())}
    other = codomain if side else domain
    plan, rows, shapes = [], [], []
    for n, (i, j) in enumerate(data.block_inds.tolist()):
        s = j if side else i
        k = where.get(tuple(space.sectors[s].tolist()))
        if k is None or new_space.block_size(k) == 0:
            continue
        recs, written = [], 0
        for tb in space.tree_blocks[s]:
            outer, A, inner, key = _split(tb, idx)
            table = mask.table(key)
            if table is None or not new_space.has_tree(tb.tree):
                continue
            k2, nb = new_space.tree_block_slice(tb.tree)
            A_dst = int(nb.multiplicities[idx])
            if k2 != k or A_dst != (mask.small(key) if large_leg else mask.large(key)) or A != (mask.large(key) if large_leg else mask.small(key)):
                raise ValueError('mask_contract: the target space does not match the mask')
            recs.append((tb.start, nb.start, outer, A, A_dst, inner, table))
            written += nb.stop - nb.start
        plan.append((n, recs, (not large_leg) or written != new_space.block_size(k)))
        rows.append((i, k) if side else (k, j))
        o = other.block_size(i if side else j)
        blk = data.blocks[n]
        shapes.append((new_space.block_size(k),) if len(blk.shape) == 1 else ((o, new_space.block_size(k)) if side else (new_space.block_size(k), o)))
    new_cod, new_dom = (codomain, new_space) if side else (new_space, domain)
    if not plan:
        return FusionTreeData(np.zeros((0, 2), np.int64), []), new_cod, new_dom
    cplx = any(_is_complex(b) for b in data.blocks)
    outs = bb.empty_many(shapes, dtype=np.complex128 if cplx else np.float64)
    records = [TreeAxisRecord(data.blocks[n], out, side, s0, d0, outer, A, A_dst, inner, table)
               for (n, recs, _), out in zip(plan, outs) for s0, d0, outer, A, A_dst, inner, table in recs]
    bb.tree_axis_many(records, 'gather' if large_leg else 'scatter', fill=[out for (_, _, z), out in zip(plan, outs) if z])
    res = FusionTreeData(np.array(rows, dtype=np.int64), outs).sorted()
    return (discard_zero_blocks(bb, res, eps) if discard else res), new_cod, new_dom


def truncated_svd(bb, a: FusionTreeData, codomain: TreeSpace, domain: TreeSpace, factors=None, **options):
    """:func:`svd`, :func:`truncate_singular_values`, and the mask applied to U's domain leg, to S and to Vh's codomain leg
    (``TensorBackend::truncated_svd``).  Returns (U, S, Vh, new_leg_space, err, new_norm).  After the SVD: the selection
    (its one download: the mask, err, new_norm) and three ``tree_axis_many`` launches reading the kept positions from the
    tables the selection left on the device -- no per-block call, no further host wait.  `factors`: the (U, S, Vh) of
    :func:`svd` of `a` where the caller already has them; they are truncated instead of decomposing again."""
    algorithm = options.pop('algorithm', None)
    common = common_sectors(codomain, domain)
    cm, dm = codomain.multiplicities, domain.multiplicities
    new_mults = [min(int(cm[i]), int(dm[j])) for i, j in common]
    U, S, Vh = factors if factors is not None else svd(bb, a, codomain, domain, new_mults, algorithm)
    sec = codomain.sectors[[i for i, _ in common]]
    keys = [tuple(x) for x in sec.tolist()]
    mid = TreeSpace.from_multiplicities(sec, [[(m,)] for m in new_mults], codomain.qdims[[i for i, _ in common]], 1,
                                        [[('svd', k)] for k in keys], [[(k,)] for k in keys])
    mask_blocks, mask_inds, err, new_norm, tables = _truncate(bb, S, mid, **options)
    mask = TreeMask.from_truncation(mask_blocks, mask_inds, mid, tables)
    J = codomain.num_legs
    U2, _, new_leg = mask_contract(bb, U, codomain, mid, mask, J, True, discard=False)
    Vh2, _, _ = mask_contract(bb, Vh, mid, domain, mask, 0, True, target=new_leg, discard=False)
    S2, _, _ = mask_contract(bb, FusionTreeData(S.block_inds[:, :1].repeat(2, axis=1), S.blocks), mid, mid, mask, 0, True,
                             target=new_leg, discard=False)
    S2 = FusionTreeData(S2.block_inds[:, :1].repeat(2, axis=1), S2.blocks)
    return U2, S2, Vh2, new_leg, err, new_norm
