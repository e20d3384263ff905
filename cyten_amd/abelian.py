"""Host side of the charge-block-sparse path: abelian sector bookkeeping around the grouped kernels.

cyten itself does not travel to the GPU box, so this module is the build's own counterpart of the
reference's ``AbelianBackend`` callers of the block backend:

* :func:`compose`  <- ``abelian_compose_worker`` (/root/reference/src/backends/abelian.cpp:1239-1469)
  The int64 sector matching (key packing, lexsort, grouping by kept legs, charge lookup, merge walk
  over contracted keys) is host work exactly as in the reference; the *hot loop* (:1424-1460) that
  issues one ``matrix_dot`` (+ ``operator+``) per matched pair is replaced by ONE grouped launch
  (`HipBlockBackend.make_gemm_plan`): each result block is one GEMM problem whose K-split pairs are
  accumulated inside the kernel.
* :func:`combine_legs_to_matrix` <- ``AbelianBackend::combine_legs`` (abelian.cpp:1022-1219):
  zero-fill + one batched strided scatter instead of ``zeros`` + ``set_item`` per block.
* :func:`svd` <- ``AbelianBackend::svd`` (abelian.cpp:3461-3568): one batched SVD over all sectors.
* :func:`truncate_singular_values` <- ``tensor_backend.cpp:139-242`` (host numpy, unchanged logic)
  + ``abelian.cpp:3623-3638``; the S blocks live in one device pool so the forced device->host
  transfer is a single copy.
* :func:`qr`, :func:`eigh` <- ``AbelianBackend::qr`` (:3084-3151), ``::eigh`` (:1759-1788).
* :func:`partial_trace`, :func:`trace_full` <- ``AbelianBackend::partial_trace`` (:2954-3081), ``::trace_full`` (:3595-3620):
  ONE grouped trace launch for all result blocks instead of ``trace_partial`` + ``operator+`` per block.
* :func:`conj`, :func:`dagger`, :class:`DiagonalTensor`, :func:`diagonal_unary`, :func:`scale_axis`, :func:`to_dense_block`,
  :func:`from_dense_block` <- ``::dagger`` (:694-703), ``::diagonal_from_block`` (:1636-1652), ``::diagonal_elementwise_unary``
  (:743-782), ``::scale_axis`` (:3178-3232), ``::to_dense_block`` (:3571-3592), ``::from_dense_block`` (:1829-1858): one batched
  launch per block list each.

* :class:`LegPipe`, :func:`combine_legs`, :func:`split_legs` <- ``AbelianLegPipe``, ``AbelianBackend::combine_legs`` (:1022-1219) behind
  the tensor level's permutation, ``::split_legs`` (:3235-3437): any number of leg groups anywhere in the tensor become pipes that
  can be contracted, decomposed and split again.  ONE launch per kernel class places all old blocks, read through their
  (permuted) strides, from a device-resident placement plan built once per block structure (``csrc/place_plan.hip``); the split
  is views, or one plan launch in reverse.
* :func:`exp`, :func:`act_block_diagonal_square_matrix`, :func:`eye`, :func:`hermitian_function` <- ``exp`` of
  ``src/tensors/ops_elementwise.cpp:174-223`` on ``AbelianBackend::act_block_diagonal_square_matrix`` (:562-593): all diagonal
  blocks of the tensor seen as a matrix of pipes go through ONE block-list call (``matrix_exp_many``: one launch of the in-LDS
  kernel ``csrc/expm_small.hip`` for the blocks that fit), instead of one block method per sector.

* :func:`outer`, :func:`tensor_from_grid`, :func:`direct_sum`, :func:`add_trivial_leg`, :func:`squeeze_legs` <-
  ``AbelianBackend::outer`` (:2794-2850), ``tensor_from_grid`` (src/tensors/constructors.cpp:304-499) on ``::from_grid`` (:1875-1978),
  ``ElementarySpace.direct_sum``, ``::add_trivial_leg`` (:596-613), ``::squeeze_legs`` (:3439-3458): what the model layer builds bond
  terms and MPO tensors from.  ALL block pairs of a tensor product go through ONE ``tensor_outer_many`` call (one launch of
  ``csrc/outer_grouped.hip``, results contiguous in their final axis order) instead of one ``tensor_outer`` per pair; a grid is one
  placement-plan launch; trivial legs are metadata.

The functions only need the block-backend *interface* (`matrix_dot_grouped`, `matrix_svd_batched`,
...), not a particular implementation.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

__all__ = ['Symmetry', 'Leg', 'AbelianTensor', 'compose', 'compose_plan', 'compose_plan_py', 'combine_legs_to_matrix', 'svd',
           'truncate_singular_values', 'truncated_svd', 'qr', 'lq', 'eigh', 'norm', 'inner', 'split_matrix_legs', 'partial_compose',
           'Mask', 'mask_contract', 'qr_tensor', 'lq_tensor', 'to_block_backend', 'move_to_device',
           'conj', 'dagger', 'DiagonalTensor', 'diagonal_unary', 'scale_axis', 'partial_trace', 'trace_full', 'to_dense_block',
           'from_dense_block', 'dual_sector_map', 'LegPipe', 'combine_legs', 'split_legs',
           'act_block_diagonal_square_matrix', 'exp', 'eye', 'hermitian_function',
           'outer', 'direct_sum', 'tensor_from_grid', 'add_trivial_leg', 'squeeze_legs']


class Symmetry:
    """Product of U(1) (modulus 0) and Z_N (modulus N) factors; sectors are int vectors."""

    def __init__(self, moduli: Sequence[int]):
        self.moduli = tuple(int(m) for m in moduli)
        self.n = len(self.moduli)

    def reduce(self, q: np.ndarray) -> np.ndarray:
        q = np.array(q, dtype=np.int64, copy=True)
        for k, m in enumerate(self.moduli):
            if m:
                q[..., k] %= m
        return q

    def fuse(self, sector_lists, signs) -> np.ndarray:
        """Row-wise sum_k signs[k]*sector_lists[k] reduced by the moduli
        (``multiple_fusion_broadcast`` of abelian.cpp:1384-1418 for abelian groups)."""
        tot = np.zeros_like(np.asarray(sector_lists[0], dtype=np.int64))
        for s, sg in zip(sector_lists, signs):
            tot = tot + sg * np.asarray(s, dtype=np.int64)
        return self.reduce(tot)

    def __eq__(self, other):
        return isinstance(other, Symmetry) and other.moduli == self.moduli

    def __repr__(self):
        return 'Symmetry(' + ' x '.join('U(1)' if m == 0 else f'Z{m}' for m in self.moduli) + ')'


def _lexsort_rows(a: np.ndarray) -> np.ndarray:
    """``np.lexsort(a.T)``: last column is the primary key (BlockInds::lexsort_indices)."""
    if a.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    return np.lexsort(a.T)


class Leg:
    """ElementarySpace mirror: sorted sectors with multiplicities, and an orientation sign
    (+1: codomain-like / incoming charge, -1: domain-like / outgoing)."""

    def __init__(self, symmetry: Symmetry, sectors, mults, sign: int = +1):
        sectors = symmetry.reduce(np.asarray(sectors, dtype=np.int64).reshape(len(mults), symmetry.n))
        mults = np.asarray(mults, dtype=np.int64)
        order = _lexsort_rows(sectors)
        self.symmetry = symmetry
        self.sectors = sectors[order]
        self.mults = mults[order]
        self.sign = int(sign)
        self.slices = np.concatenate([[0], np.cumsum(self.mults)])

    @property
    def nsec(self):
        return len(self.mults)

    @property
    def dim(self):
        return int(self.mults.sum())

    def dual(self) -> 'Leg':
        return Leg(self.symmetry, self.sectors, self.mults, -self.sign)

    def can_contract_with(self, other: 'Leg') -> bool:
        return (self.sign == -other.sign and np.array_equal(self.sectors, other.sectors)
                and np.array_equal(self.mults, other.mults))

    def __repr__(self):
        return f'Leg(nsec={self.nsec}, dim={self.dim}, sign={self.sign:+d})'


@dataclass
class AbelianTensor:
    """AbelianBackendData mirror (/root/reference/include/cyten/backends/abelian.h:52-83): a list
    of dense blocks plus the int64 table ``block_inds`` (one row per block, one column per leg,
    entries = sector index on that leg), lexsorted.  Charge rule: sum_k sign_k * q_k = 0."""
    symmetry: Symmetry
    legs: list
    blocks: list
    block_inds: np.ndarray
    num_codomain: int = 0
    labels: list = field(default_factory=list)
    ptrs: np.ndarray = field(default=None, repr=False, compare=False)   # device addresses of the blocks when they are C-contiguous
                                                                         # float64 arrays (None: not known / not the case)

    def __post_init__(self):
        self.block_inds = np.asarray(self.block_inds, dtype=np.int64).reshape(len(self.blocks), len(self.legs))

    def block_ptrs(self):
        """int64 array of the blocks' device addresses if every block is a C-contiguous float64 device block (computed once per
        tensor), else None: the table `cyb_compose_plan_enqueue_f64` and the placement launches read instead of block objects"""
        if self.ptrs is None:
            try:
                ok = all(b.is_contiguous() and not b.is_complex and not b.is_bool and getattr(b, '_nom', None) is None for b in self.blocks)
            except AttributeError:      # (blocks of another backend, e.g. numpy arrays)
                return None
            if not ok:
                return None
            self.ptrs = np.fromiter((b.ptr for b in self.blocks), dtype=np.int64, count=len(self.blocks))
        return self.ptrs

    @property
    def nlegs(self):
        return len(self.legs)

    def sorted(self) -> 'AbelianTensor':
        order = _lexsort_rows(self.block_inds)
        return AbelianTensor(self.symmetry, self.legs, [self.blocks[i] for i in order], self.block_inds[order],
                             self.num_codomain, self.labels, None if self.ptrs is None else self.ptrs[order])

    def block_shape(self, row) -> tuple:
        return tuple(int(l.mults[i]) for l, i in zip(self.legs, row))

    def check_charges(self):
        for row in self.block_inds:
            q = self.symmetry.fuse([l.sectors[i] for l, i in zip(self.legs, row)], [l.sign for l in self.legs])
            if np.any(q != 0):
                raise ValueError(f'block {row} violates the charge rule')

    @staticmethod
    def allowed_block_inds(symmetry, legs) -> np.ndarray:
        """All sector-index combinations with total charge 0 (lexsorted)."""
        grids = np.indices([l.nsec for l in legs]).reshape(len(legs), -1).T
        if grids.shape[0] == 0:
            return grids.astype(np.int64)
        q = symmetry.fuse([l.sectors[grids[:, k]] for k, l in enumerate(legs)], [l.sign for l in legs])
        ok = np.all(q == 0, axis=1)
        inds = grids[ok].astype(np.int64)
        return inds[_lexsort_rows(inds)]

    @classmethod
    def from_numpy_blocks(cls, bb, symmetry, legs, np_blocks, block_inds, num_codomain=0):
        return cls(symmetry, list(legs), [bb.as_block(b) for b in np_blocks], block_inds, num_codomain).sorted()

    @classmethod
    def from_spec(cls, bb, spec):
        """Upload a plain-data tensor (``cyten_amd.workloads.TensorSpec``: moduli, legs with
        sectors/mults/sign, block_inds, numpy blocks) to the device."""
        sym = Symmetry(spec.moduli)
        legs = [Leg(sym, l.sectors, l.mults, l.sign) for l in spec.legs]
        return cls.from_numpy_blocks(bb, sym, legs, spec.blocks, spec.block_inds, spec.num_codomain)

    def to_numpy_blocks(self, bb):
        return [bb.to_numpy(b) for b in self.blocks]

    def to_dense(self, bb) -> np.ndarray:
        """Dense array (test helper; the reference tests compare against ``.to_numpy()``)."""
        cplx = any(getattr(b, 'dtype', np.dtype('float64')).kind == 'c' for b in self.blocks)
        out = np.zeros([l.dim for l in self.legs], dtype=np.complex128 if cplx else np.float64)
        for blk, row in zip(self.blocks, self.block_inds):
            sl = tuple(slice(int(l.slices[i]), int(l.slices[i + 1])) for l, i in zip(self.legs, row))
            out[sl] = bb.to_numpy(blk)
        return out


# ---------------------------------------------------------------------------------------------
# compose / tdot
# ---------------------------------------------------------------------------------------------

@dataclass
class ComposePlan:
    """Result of the host-side sector matching: which (a-block, b-block) pairs feed which result
    block.  ``pairs[g]`` lists (index into a.blocks, index into b.blocks) for result block g."""
    res_block_inds: np.ndarray
    res_shapes: list
    pairs: list
    legs: list
    flops: float = 0.0
    native: object = None      # the library's plan object (kept for `cyb_compose_plan_enqueue_f64`), or None
    shapes_np: np.ndarray = None


class _NativePlan:
    """owner of a `cyb_compose_plan_t`"""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle

    def __del__(self):
        try:
            self.lib.cyb_compose_plan_destroy(self.handle)
        except Exception:
            pass


_PLAN_CACHE: dict = {}


_native = None  # (lib, check) once libcyten_amd has been loaded; False if it cannot be


def _native_planner():
    global _native
    if _native is None:
        try:
            from . import _lib
            _native = (_lib.load(), _lib)
        except (ImportError, OSError):
            _native = False
    return _native


def _leg_descs(legs):
    """ctypes view of a leg list for the C++ planner (arrays kept alive by the returned tuple)."""
    _, L = _native
    arr = (L.LegDesc * max(len(legs), 1))()
    keep = []
    for i, lg in enumerate(legs):
        sec = np.ascontiguousarray(lg.sectors, dtype=np.int64)
        mul = np.ascontiguousarray(lg.mults, dtype=np.int64)
        keep += [sec, mul]
        arr[i].n_sectors, arr[i].sectors, arr[i].mults, arr[i].sign = lg.nsec, sec.ctypes.data, mul.ctypes.data, lg.sign
    return arr, keep


def compose_plan(a: AbelianTensor, b: AbelianTensor, num_contr: int) -> ComposePlan:
    """Sector matching of ``abelian_compose_worker`` (abelian.cpp:1265-1460): the C++ planner of
    ``csrc/abelian_plan.hip`` (``cyb_compose_plan_create``) when the library is built, else -- and as the specification
    the tests compare it with -- :func:`compose_plan_py`."""
    nat = _native_planner()
    if not nat or a.symmetry != b.symmetry:
        return compose_plan_py(a, b, num_contr)
    for i in range(min(num_contr, a.nlegs, b.nlegs)):   # (the C++ planner compares sectors; pipes also need the same internal order)
        if isinstance(a.legs[a.nlegs - 1 - i], LegPipe) and not a.legs[a.nlegs - 1 - i].can_contract_with(b.legs[i]):
            raise ValueError(f'legs a[{a.nlegs - 1 - i}] and b[{i}] are not contractible')
    # the matching depends on the legs and the two block tables only: cached by content like the placement tables of
    # combine_legs (the same structures come back bond after bond, sweep after sweep)
    key = (_legs_key(a.symmetry, a.legs, [l.sign for l in a.legs]), _legs_key(b.symmetry, b.legs, [l.sign for l in b.legs]), num_contr,
           a.block_inds.shape, a.block_inds.tobytes(), b.block_inds.shape, b.block_inds.tobytes())
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        return hit
    import ctypes as C
    lib, L = nat
    na_keep, nb_keep = a.nlegs - num_contr, b.nlegs - num_contr
    if na_keep < 0 or nb_keep < 0:
        return compose_plan_py(a, b, num_contr)
    res_legs = list(a.legs[:na_keep]) + list(b.legs[num_contr:])
    la, keep_a = _leg_descs(a.legs)
    lb, keep_b = _leg_descs(b.legs)
    abi = np.ascontiguousarray(a.block_inds, dtype=np.int64)
    bbi = np.ascontiguousarray(b.block_inds, dtype=np.int64)
    mod = np.array(a.symmetry.moduli, dtype=np.int64)
    handle = C.c_void_p()
    L.check(lib.cyb_compose_plan_create(mod.ctypes.data, a.symmetry.n, la, a.nlegs, abi.ctypes.data, len(a.blocks), lb, b.nlegs,
                                        bbi.ctypes.data, len(b.blocks), num_contr, C.byref(handle)))
    try:
        n_res, n_pairs, n_cols = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(lib.cyb_compose_plan_sizes(handle, C.byref(n_res), C.byref(n_pairs), C.byref(n_cols)))
        nr, npair, nc = n_res.value, n_pairs.value, n_cols.value
        res_bi = np.zeros((nr, nc), dtype=np.int64)
        shapes = np.zeros((nr, nc), dtype=np.int64)
        goff = np.zeros(nr + 1, dtype=np.int64)
        pa, pb = np.zeros(max(npair, 1), dtype=np.int64), np.zeros(max(npair, 1), dtype=np.int64)
        flops = C.c_double()
        L.check(lib.cyb_compose_plan_get(handle, res_bi.ctypes.data, shapes.ctypes.data, goff.ctypes.data, pa.ctypes.data,
                                         pb.ctypes.data, C.byref(flops)))
    except Exception:
        lib.cyb_compose_plan_destroy(handle)
        raise
    pal, pbl, gl = pa.tolist(), pb.tolist(), goff.tolist()
    pairs = [list(zip(pal[gl[g]:gl[g + 1]], pbl[gl[g]:gl[g + 1]])) for g in range(nr)]
    plan = ComposePlan(res_bi, [tuple(r) for r in shapes.tolist()], pairs, res_legs, flops.value, _NativePlan(lib, handle), shapes)
    return _cache_put(_PLAN_CACHE, key, plan)


def compose_plan_py(a: AbelianTensor, b: AbelianTensor, num_contr: int) -> ComposePlan:
    """Sector matching of ``abelian_compose_worker`` (abelian.cpp:1265-1460), int64 host work in numpy.

    Contracts the last `num_contr` legs of `a` with the first `num_contr` legs of `b`; as in the
    reference's leg layout (legs = codomain + reversed domain) a's contracted legs appear in
    REVERSED order relative to b's: ``a.legs[-1-i]`` pairs with ``b.legs[i]``."""
    na_keep = a.nlegs - num_contr
    for i in range(num_contr):
        if not a.legs[a.nlegs - 1 - i].can_contract_with(b.legs[i]):
            raise ValueError(f'legs a[{a.nlegs - 1 - i}] and b[{i}] are not contractible')
    res_legs = list(a.legs[:na_keep]) + list(b.legs[num_contr:])
    nb_keep = b.nlegs - num_contr
    empty = ComposePlan(np.zeros((0, na_keep + nb_keep), np.int64), [], [], res_legs)
    if len(a.blocks) == 0 or len(b.blocks) == 0:
        return empty
    a_keep, a_contr = a.block_inds[:, :na_keep], a.block_inds[:, na_keep:]
    b_contr, b_keep = b.block_inds[:, :num_contr], b.block_inds[:, num_contr:]
    # pack the contracted columns into one key, F-style strides over b's leg order (:1265-1283)
    nsecs = [b.legs[i].nsec for i in range(num_contr)]
    strides = np.ones(num_contr, dtype=np.int64)
    for i in range(1, num_contr):
        strides[i] = strides[i - 1] * nsecs[i - 1]
    a_keys = a_contr @ strides[::-1] if num_contr else np.zeros(len(a.blocks), np.int64)
    b_keys = b_contr @ strides if num_contr else np.zeros(len(b.blocks), np.int64)
    # sort a by (keep columns, contracted key): np.lexsort(hstack([key, keep]).T)  (:1286-1303)
    a_sort = _lexsort_rows(np.hstack([a_keys[:, None], a_keep]))
    a_keep, a_keys = a_keep[a_sort], a_keys[a_sort]
    # b is lexsorted already (last column primary) => grouped by its keep columns with ascending keys
    b_sort = _lexsort_rows(np.hstack([b_keys[:, None], b_keep]))
    b_keep, b_keys = b_keep[b_sort], b_keys[b_sort]

    def row_groups(keep):
        if keep.shape[1] == 0:
            return np.array([0, keep.shape[0]])
        diff = np.any(keep[1:] != keep[:-1], axis=1)
        return np.concatenate([[0], np.flatnonzero(diff) + 1, [keep.shape[0]]])

    a_sl, b_sl = row_groups(a_keep), row_groups(b_keep)
    a_rows, b_cols = a_keep[a_sl[:-1]], b_keep[b_sl[:-1]]
    # coupled charge of the kept legs of every row of a / column of b (:1384-1418)
    sym = a.symmetry
    if na_keep:
        a_ch = sym.fuse([a.legs[k].sectors[a_rows[:, k]] for k in range(na_keep)], [a.legs[k].sign for k in range(na_keep)])
    else:
        a_ch = np.zeros((len(a_rows), sym.n), np.int64)
    if nb_keep:
        b_ch = sym.fuse([b.legs[num_contr + k].sectors[b_cols[:, k]] for k in range(nb_keep)],
                        [-b.legs[num_contr + k].sign for k in range(nb_keep)])
    else:
        b_ch = np.zeros((len(b_cols), sym.n), np.int64)
    lookup: dict = {}
    for r, ch in enumerate(map(tuple, a_ch)):  # cyten.tools.misc.list_to_dict_list (:1420)
        lookup.setdefault(ch, []).append(r)

    res_rows, res_shapes, pairs = [], [], []
    flops = 0.0
    for cb in range(len(b_cols)):
        kb = b_keys[b_sl[cb]:b_sl[cb + 1]]
        for ra in lookup.get(tuple(b_ch[cb]), []):
            ka = a_keys[a_sl[ra]:a_sl[ra + 1]]
            common, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)  # merge walk (:1430)
            if len(common) == 0:
                continue
            grp = [(int(a_sort[a_sl[ra] + i]), int(b_sort[b_sl[cb] + j])) for i, j in zip(ia, ib)]
            row = np.concatenate([a_rows[ra], b_cols[cb]])
            shp = tuple(int(res_legs[k].mults[row[k]]) for k in range(len(row)))
            res_rows.append(row)
            res_shapes.append(shp)
            pairs.append(grp)
            M = math.prod(map(int, shp[:na_keep]))
            N = math.prod(map(int, shp[na_keep:]))
            for ai, _ in grp:
                K = math.prod(map(int, a.block_shape(a.block_inds[ai])[na_keep:]))
                flops += 2.0 * M * N * K
    if not res_rows:
        return empty
    res_bi = np.array(res_rows, dtype=np.int64).reshape(len(res_rows), na_keep + nb_keep)
    order = _lexsort_rows(res_bi)
    return ComposePlan(res_bi[order], [res_shapes[i] for i in order], [pairs[i] for i in order], res_legs, flops)


def _compose_operands(bb, a, b, num_contr, plan):
    """2-D operand views for every block that takes part (reshape :1349-1382).  b-blocks need
    their contracted axes reversed; when that is not a stride-mergeable view all such blocks are
    made contiguous in ONE batched copy."""
    na_keep = a.nlegs - num_contr
    used_a = sorted({i for g in plan.pairs for i, _ in g})
    used_b = sorted({j for g in plan.pairs for _, j in g})
    a2 = {}
    a_src = bb.contiguous_many([a.blocks[i] for i in used_a])
    for i, blk in zip(used_a, a_src):
        rows = math.prod(map(int, blk.shape[:na_keep]))
        a2[i] = bb.reshape(blk, (rows, -1))
    perm = list(range(num_contr - 1, -1, -1)) + list(range(num_contr, b.nlegs))
    b_perm = [bb.permute_axes(b.blocks[j], perm) for j in used_b]
    b_perm = bb.contiguous_many(b_perm)  # no-op (no launch) when nothing was permuted
    b2 = {}
    for j, blk in zip(used_b, b_perm):
        cols = math.prod(map(int, blk.shape[num_contr:]))
        b2[j] = bb.reshape(blk, (-1, cols))
    return a2, b2


def make_compose_gemm(bb, a: AbelianTensor, b: AbelianTensor, num_contr: int, plan: ComposePlan | None = None):
    """Build the device launch plan of one contraction: returns (ComposePlan, GemmPlan)."""
    if plan is None:
        plan = compose_plan(a, b, num_contr)
    a2, b2 = _compose_operands(bb, a, b, num_contr, plan)
    groups = [[(a2[i], b2[j]) for i, j in g] for g in plan.pairs]
    return plan, (bb.make_gemm_plan(groups) if groups else None)


class LazyBlocks:
    """The result blocks of a block-list operation as views into ONE buffer, created when somebody asks for them: the hot
    path hands address tables from launch to launch and never looks at most blocks as objects (728 of them per U(1)xU(1)
    theta)."""

    def __init__(self, bb, buf, offsets, shapes):
        self.bb, self.buf, self.offsets, self.shapes = bb, buf, offsets, shapes
        self._made = [None] * len(shapes)

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        blk = self._made[i]
        if blk is None:
            from .block_backend import HipBlock, _c_strides
            sh = tuple(int(x) for x in self.shapes[i])
            blk = self._made[i] = HipBlock._trusted(self.bb, self.buf, int(self.offsets[i]), sh, _c_strides(sh), True)
        return blk

    def __iter__(self):
        return (self[i] for i in range(len(self)))


def compose_enqueue(bb, plan: ComposePlan, a_ptrs, b_ptrs, out_ptrs, which=None):
    """`cyb_compose_plan_enqueue_f64`: the contraction of `plan` for operand blocks given as address tables, results at
    `out_ptrs` (one per entry of `which`, default all result blocks).  Returns (flops, bytes) of what was enqueued."""
    import ctypes as C
    _, L = _native
    fl, by = C.c_double(), C.c_double()
    out_ptrs = np.ascontiguousarray(out_ptrs, dtype=np.int64)
    w = None if which is None else np.ascontiguousarray(which, dtype=np.int64)
    bb.ctx.sync_stream()
    L.check(bb.lib.cyb_compose_plan_enqueue_f64(bb.ctx.handle, plan.native.handle, a_ptrs.ctypes.data, b_ptrs.ctypes.data,
                                                None if w is None else w.ctypes.data, 0 if w is None else len(w), out_ptrs.ctypes.data,
                                                C.byref(fl), C.byref(by)))
    return fl.value, by.value


def _compose_native(bb, a, b, num_contr, plan):
    """the whole contraction behind the C-ABI (descriptors built in the library), for C-contiguous float64 device blocks"""
    if plan.native is None or num_contr > 1 or not hasattr(bb, 'lib'):
        return None
    pa, pb = a.block_ptrs(), b.block_ptrs()
    if pa is None or pb is None:
        return None
    shapes = plan.shapes_np
    sizes = shapes.prod(axis=1) if shapes.shape[1] else np.ones(len(shapes), dtype=np.int64)
    padded = (sizes + 31) // 32 * 32
    offs = np.concatenate([[0], np.cumsum(padded)[:-1]])
    buf = bb.ctx.empty(int(padded.sum()))
    out_ptrs = buf.data_ptr() + 8 * offs
    compose_enqueue(bb, plan, pa, pb, out_ptrs)
    return AbelianTensor(a.symmetry, plan.legs, LazyBlocks(bb, buf, offs, plan.res_shapes), plan.res_block_inds, a.nlegs - num_contr,
                         ptrs=out_ptrs)


def compose(bb, a: AbelianTensor, b: AbelianTensor, num_contr: int) -> AbelianTensor:
    """Contract the last `num_contr` legs of a with the first `num_contr` legs of b."""
    plan = compose_plan(a, b, num_contr)
    na_keep = a.nlegs - num_contr
    if not plan.pairs:
        return AbelianTensor(a.symmetry, plan.legs, [], plan.res_block_inds, na_keep)
    fast = _compose_native(bb, a, b, num_contr, plan)
    if fast is not None:
        return fast
    a2, b2 = _compose_operands(bb, a, b, num_contr, plan)
    outs = bb.matrix_dot_grouped([[(a2[i], b2[j]) for i, j in g] for g in plan.pairs])
    blocks = [bb.reshape(o, shp) for o, shp in zip(outs, plan.res_shapes)]
    return AbelianTensor(a.symmetry, plan.legs, blocks, plan.res_block_inds, na_keep)


# ---------------------------------------------------------------------------------------------
# combine legs -> matrix, decompositions
# ---------------------------------------------------------------------------------------------

@dataclass
class MatrixView:
    """A tensor with its first `num_codomain` legs fused into a row leg and the rest into a column
    leg: one 2-D block per coupled charge (the form ``AbelianBackend::svd/qr/eigh`` work on)."""
    symmetry: Symmetry
    charges: np.ndarray      # (n_sectors, n_sym) coupled charge of each block
    blocks: list             # 2-D blocks (rows, cols)
    row_maps: list           # per sector: list of (leg-index tuple over the row legs, row slice start, size)
    col_maps: list
    row_legs: list
    col_legs: list


# Fusion maps and placement tables depend on the legs (and the block table) only, and the same combinations come back bond after
# bond, sweep after sweep: they are cached by CONTENT (the reference keeps the same tables inside its LegPipe objects,
# abelian.cpp:1022-1219, which live as long as the legs do).  Small bounded dictionaries, oldest entries dropped first.
_FUSE_CACHE: dict = {}
_PLACE_CACHE: dict = {}
_CACHE_MAX = 256


def _cache_put(cache, key, value):
    if len(cache) >= _CACHE_MAX:
        cache.pop(next(iter(cache)))
    cache[key] = value
    return value


def _legs_key(symmetry, legs, signs):
    return (symmetry.moduli,) + tuple((l.sectors.tobytes(), l.mults.tobytes(), int(sg)) for l, sg in zip(legs, signs))


def _fused_sector_maps(symmetry, legs, signs_override=None):
    """All sector-index combinations of `legs`, grouped by coupled charge:
    {charge tuple: [(index tuple, offset, size), ...]} in lexsorted (C-style) order
    (LegPipe fusion of abelian.cpp:1022-1219).  Cached; callers must not modify the result."""
    if not legs:
        return {tuple([0] * symmetry.n): [((), 0, 1)]}
    key = _legs_key(symmetry, legs, [l.sign for l in legs] if signs_override is None else signs_override)
    hit = _FUSE_CACHE.get(key)
    if hit is not None:
        return hit
    return _cache_put(_FUSE_CACHE, key, _fused_sector_maps_build(symmetry, legs, signs_override))


def _fused_sector_maps_build(symmetry, legs, signs_override=None):
    grids = np.indices([l.nsec for l in legs]).reshape(len(legs), -1).T
    signs = [l.sign for l in legs] if signs_override is None else signs_override
    q = symmetry.fuse([l.sectors[grids[:, k]] for k, l in enumerate(legs)], signs)
    sizes = np.prod([l.mults[grids[:, k]] for k, l in enumerate(legs)], axis=0)
    out: dict = {}
    for idx, ch, sz in zip(map(tuple, grids), map(tuple, q), sizes):
        lst = out.setdefault(ch, [])
        off = lst[-1][1] + lst[-1][2] if lst else 0
        lst.append((tuple(int(i) for i in idx), int(off), int(sz)))
    return out


def combine_legs_to_matrix(bb, t: AbelianTensor, num_codomain: int | None = None) -> MatrixView:
    """Fuse legs[:num_codomain] into rows and legs[num_codomain:] into columns.

    Reference: ``AbelianBackend::combine_legs`` allocates ``bb.zeros`` per result block and writes
    every old block with ``new_block[slices] = combined`` (abelian.cpp:1196-1217).  Here: ONE
    allocation + memset for the result block list and ONE batched strided scatter."""
    nc = t.num_codomain if num_codomain is None else num_codomain
    row_legs, col_legs = t.legs[:nc], t.legs[nc:]
    sym = t.symmetry
    binds = np.ascontiguousarray(t.block_inds, dtype=np.int64)
    # ---- placement table: which old block goes where in which coupled-charge matrix (legs and block table only: cached)
    key = (_legs_key(sym, row_legs, [l.sign for l in row_legs]), _legs_key(sym, col_legs, [-l.sign for l in col_legs]), nc,
           binds.shape, binds.tobytes())
    plan = _PLACE_CACHE.get(key)
    if plan is None:
        rmap = _fused_sector_maps(sym, row_legs)
        # column charge is defined so that row charge == column charge for an allowed block
        cmap = _fused_sector_maps(sym, col_legs, [-l.sign for l in col_legs])
        rpos = {ch: {idx: (off, sz) for idx, off, sz in lst} for ch, lst in rmap.items()}
        cpos = {ch: {idx: (off, sz) for idx, off, sz in lst} for ch, lst in cmap.items()}
        present: dict = {}
        if nc and len(binds):  # coupled charge of the row legs of every block at once
            ch_all = sym.fuse([l.sectors[binds[:, k]] for k, l in enumerate(row_legs)], [l.sign for l in row_legs]).tolist()
        else:
            ch_all = [[0] * sym.n] * len(binds)
        for bi, (row, ch) in enumerate(zip(binds.tolist(), ch_all)):
            present.setdefault(tuple(ch), []).append((bi, tuple(row[:nc]), tuple(row[nc:])))
        charges = sorted(present.keys(), key=lambda c: tuple(reversed(c)))
        n = len(binds)
        big_of, ro_a, co_a, rs_a, cs_a = (np.zeros(n, dtype=np.int64) for _ in range(5))
        for gi, ch in enumerate(charges):
            rp, cp = rpos[ch], cpos[ch]
            for bi, ridx, cidx in present[ch]:
                ro, rs = rp[ridx]
                co, cs = cp[cidx]
                big_of[bi], ro_a[bi], co_a[bi], rs_a[bi], cs_a[bi] = gi, ro, co, rs, cs
        shapes = [(sum(sz for _, _, sz in rmap[ch]), sum(sz for _, _, sz in cmap[ch])) for ch in charges]
        plan = _cache_put(_PLACE_CACHE, key, dict(
            charges=np.array(charges, dtype=np.int64).reshape(len(charges), sym.n), shapes=shapes, big_of=big_of, ro=ro_a, co=co_a,
            rs=rs_a, cs=cs_a, row_maps=[rmap[ch] for ch in charges], col_maps=[cmap[ch] for ch in charges]))
    shapes, big_of, ro_a, co_a, rs_a, cs_a = plan['shapes'], plan['big_of'], plan['ro'], plan['co'], plan['rs'], plan['cs']
    row_maps, col_maps = list(plan['row_maps']), list(plan['col_maps'])
    src_ptrs = t.block_ptrs() if (hasattr(bb, 'copy_2d_many') and len(binds) > 0) else None   # (float64, C-contiguous: the address table)
    cplx = src_ptrs is None and any(np.dtype(getattr(blk, 'dtype', np.float64)).kind == 'c' for blk in t.blocks)
    blocks = bb.zeros_many(shapes, dtype='complex128' if cplx else None)
    sub = getattr(bb, 'subblock', None)  # (a backend may offer the 2-D slice without the generality of get_item)
    if src_ptrs is not None:
        # placement as plain arrays (address, leading dimension, extents) per old block: one descriptor array filled by
        # numpy and one launch, no view objects per block (the 728-block U(1)xU(1) theta: 8 -> 2 ms of host time)
        base = np.array([b.ptr for b in blocks], dtype=np.int64)
        ld = plan.get('ld')
        if ld is None:
            ld = plan['ld'] = np.array([sh[1] for sh in shapes], dtype=np.int64)
        dptr = base[big_of] + 8 * (ro_a * ld[big_of] + co_a)
        bb.copy_2d_many(dptr, ld[big_of], src_ptrs, cs_a, rs_a, cs_a)
    else:
        pairs = []
        for bi in range(len(binds)):
            big = blocks[int(big_of[bi])]
            ro, co, rs, cs = int(ro_a[bi]), int(co_a[bi]), int(rs_a[bi]), int(cs_a[bi])
            target = sub(big, ro, ro + rs, co, co + cs) if sub else bb.get_item(big, (slice(ro, ro + rs), slice(co, co + cs)))
            pairs.append((target, bb.reshape(t.blocks[bi], (rs, cs))))
        bb.copy_many(pairs)
    charges = plan['charges'].copy()
    return MatrixView(sym, charges, blocks, row_maps, col_maps,
                      list(row_legs), list(col_legs))


def svd(bb, mv: MatrixView, algorithm=None):
    """Thin SVD of every coupled-charge block in ONE batched call (abelian.cpp:3499-3541).
    Returns lists U, S, Vh (per sector)."""
    res = bb.matrix_svd_batched(mv.blocks, algorithm)
    return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]


def qr(bb, mv: MatrixView, full=False):
    res = bb.matrix_qr_batched(mv.blocks, full)
    return [r[0] for r in res], [r[1] for r in res]


def lq(bb, mv: MatrixView, full=False):
    """L, Q of every coupled-charge block in ONE batched call (the per-block ``matrix_lq`` of ``AbelianBackend::lq``,
    abelian.cpp:2304-2385; block_backend.cpp:1033-1040: QR of the transposed view)."""
    res = bb.matrix_lq_batched(mv.blocks, full)
    return [r[0] for r in res], [r[1] for r in res]


def eigh(bb, mv: MatrixView, sort=None):
    res = bb.eigh_batched(mv.blocks, sort)
    return [r[0] for r in res], [r[1] for r in res]


def truncation_selection(S: np.ndarray, qdims=None, chi_max=None, chi_min=1, degeneracy_tol=0.0, trunc_cut=0.0,
                         svd_min=None, minimize_error=True):
    """Which singular values to keep: mirror of
    ``TensorBackend::_truncate_singular_values_selection`` (tensor_backend.cpp:139-242), pure host
    numpy like the reference.  Returns (mask, err, new_norm)."""
    S = np.asarray(S, dtype=np.float64)
    marginal = S ** 2 if qdims is None else np.asarray(qdims) * S ** 2
    piv = np.argsort(marginal, kind='stable')
    S_s, marg = S[piv], marginal[piv]
    logS = np.log(np.where(S_s <= 1e-100, 1e-100, S_s))
    n = len(S_s)
    good = np.ones(n, dtype=bool)

    def combine(good, good2):
        both = good & good2
        return both if both.any() else good  # keep the previous constraint set if incompatible

    if chi_max is not None and chi_max < n:
        g2 = np.zeros(n, dtype=bool)
        g2[-chi_max:] = True
        good = combine(good, g2)
    if chi_min > 1:
        g2 = np.ones(n, dtype=bool)
        g2[-chi_min + 1:] = False
        good = combine(good, g2)
    if degeneracy_tol > 0:
        g2 = np.empty(n, dtype=bool)
        g2[0] = True
        g2[1:] = (logS[1:] - logS[:-1]) >= degeneracy_tol
        good = combine(good, g2)
    if svd_min is not None:
        good = combine(good, S_s >= svd_min)
    good = combine(good, np.cumsum(marg) > trunc_cut * trunc_cut)
    nz = np.flatnonzero(good)
    cut = int(nz[0] if minimize_error else nz[-1])
    err = float(np.sum(marg[:cut]))
    new_norm = float(np.sum(marg[cut:]))
    mask = np.zeros(n, dtype=bool)
    mask[piv[cut:]] = True
    return mask, err, new_norm


def truncate_singular_values(bb, S_blocks, **options):
    """Pull all singular values to the host (the reference's forced sync point,
    abelian.cpp:3631), select, and return per-sector boolean masks + (err, new_norm)."""
    sizes = [s.size for s in S_blocks]
    if hasattr(bb, 'concatenate_to_numpy'):  # one gather launch + one download instead of one download per sector
        S_all = bb.concatenate_to_numpy(S_blocks)
    else:
        S_all = np.concatenate([bb.to_numpy(s) for s in S_blocks]) if S_blocks else np.zeros(0)
    mask, err, new_norm = truncation_selection(S_all, **options)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    return [mask[offs[i]:offs[i + 1]] for i in range(len(sizes))], err, new_norm


def truncated_svd(bb, theta: AbelianTensor, num_codomain=None, lazy_null=False, **options):
    """combine -> batched SVD -> truncation -> batched mask gather (decompositions.cpp:673-712).  With a backend that
    offers ``truncate_select`` the selection runs on the device and the gather reads the kept positions from there
    (the host sees the kept counts, err and new_norm only); otherwise -- and for lists beyond the device limit -- the
    reference's host selection on the downloaded singular values.

    ``lazy_null=True``: the singular vectors of numerically zero singular values are only computed if the truncation
    keeps them.  Every block of a two-site theta = A.B is rank-deficient, and ``svd_apply_mask`` (decompositions.cpp:620-631)
    throws those vectors away; the first SVD call skips their orthonormal completion (``CYB_SVD_SKIP_NULL_VECTORS``) and
    reports the numerical ranks, and only a sector whose kept count exceeds its rank -- ``chi_max`` beyond the number of
    non-zero singular values -- is decomposed again in full.  The returned factors are those of the eager path."""
    mv = combine_legs_to_matrix(bb, theta, num_codomain)
    ranks = None
    if lazy_null and hasattr(bb, 'lib'):
        res, ranks = bb.matrix_svd_batched(mv.blocks, null_vectors=False, return_rank=True)
        U, S, Vh = [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]
    else:
        U, S, Vh = svd(bb, mv)
    masks = None
    if hasattr(bb, 'truncate_select') and 0 < sum(s.size for s in S) <= bb.TRUNCATE_MAX:
        try:    # (quantum-dimension weights: one per sector, or per value and constant inside a sector -- else host work)
            masks, _, err, new_norm = bb.truncate_select(S, **options)
        except NotImplementedError:
            masks = None
    if masks is None:
        masks, err, new_norm = truncate_singular_values(bb, S, **options)
    if ranks is not None:   # sectors that keep a deflated singular value need their null vectors after all
        kept = [int(m.n if hasattr(m, 'n') else np.count_nonzero(m)) for m in masks]
        redo = [i for i, (k, r) in enumerate(zip(kept, ranks)) if k > r]
        if redo:
            full = bb.matrix_svd_batched([mv.blocks[i] for i in redo])
            for i, (u, s, vh) in zip(redo, full):
                U[i], S[i], Vh[i] = u, s, vh
    gathered = bb.mask_gather_many([(u, m, 1) for u, m in zip(U, masks)] + [(s, m, 0) for s, m in zip(S, masks)]
                                   + [(v, m, 0) for v, m in zip(Vh, masks)])
    n = len(U)
    return mv, gathered[:n], gathered[n:2 * n], gathered[2 * n:], err, new_norm


def split_matrix_legs(bb, mv: MatrixView, blocks, side: str):
    """Split the fused row ('rows': U-like blocks (rows, k)) or column ('cols': Vh-like (k, cols))
    leg back into the original legs (abelian.cpp:3414-3434 does get_item+reshape per block).
    Row slices are views; the column slices of all sectors are made contiguous by ONE batched gather."""
    if side not in ('rows', 'cols'):
        raise ValueError(f"side must be 'rows' or 'cols', got {side!r}")
    out, subs = [], []
    for sec, blk in enumerate(blocks):
        maps = mv.row_maps[sec] if side == 'rows' else mv.col_maps[sec]
        legs = mv.row_legs if side == 'rows' else mv.col_legs
        for idx, off, sz in maps:
            dims = [int(l.mults[i]) for l, i in zip(legs, idx)]
            if side == 'rows':
                sub = bb.get_item(blk, (slice(off, off + sz), slice(None)))
                out.append((sec, idx, bb.reshape(sub, dims + [blk.shape[1]])))
            else:
                subs.append(bb.get_item(blk, (slice(None), slice(off, off + sz))))
                out.append((sec, idx, [blk.shape[0]] + dims))
    if side == 'cols':
        dense = bb.contiguous_many(subs)
        out = [(sec, idx, bb.reshape(d, shape)) for (sec, idx, shape), d in zip(out, dense)]
    return out


def norm(bb, t: AbelianTensor) -> float:
    """abelian.cpp:2781-2792: one reduction over the whole block list."""
    return bb.norm_many(t.blocks)


def inner(bb, a: AbelianTensor, b: AbelianTensor) -> float:
    """abelian.cpp:2159-2211: <a|b> over the blocks present in both (same legs)."""
    ia = {tuple(r): i for i, r in enumerate(a.block_inds)}
    xs, ys = [], []
    for j, r in enumerate(b.block_inds):
        i = ia.get(tuple(r))
        if i is not None:
            xs.append(a.blocks[i])
            ys.append(b.blocks[j])
    return bb.inner_many(xs, ys)


# ---------------------------------------------------------------------------------------------
# leg permutation and vector-space operations (what the Krylov solvers need between composes)
# ---------------------------------------------------------------------------------------------

def permute_legs(bb, t: AbelianTensor, perm: Sequence[int], num_codomain: int | None = None) -> AbelianTensor:
    """Reorder the legs (AbelianBackend::permute_legs, abelian.cpp:2860-2905, without leg bending:
    signs stay with their legs).  Blocks become strided views (no data movement here: the next
    compose makes the operands it needs contiguous in one batched copy), the block table is
    re-sorted."""
    perm = [int(p) for p in perm]
    if sorted(perm) != list(range(t.nlegs)):
        raise ValueError(f'permute_legs: {perm} is not a permutation of {t.nlegs} legs')
    legs = [t.legs[p] for p in perm]
    blocks = [bb.permute_axes(b, perm) for b in t.blocks]
    out = AbelianTensor(t.symmetry, legs, blocks, t.block_inds[:, perm] if len(blocks) else t.block_inds.reshape(0, t.nlegs),
                        t.num_codomain if num_codomain is None else num_codomain)
    return out.sorted()


def _align(a: AbelianTensor, b: AbelianTensor):
    if a.nlegs != b.nlegs or any(x.nsec != y.nsec or x.sign != y.sign for x, y in zip(a.legs, b.legs)):
        raise ValueError('tensors live on different legs')
    ia = {tuple(r): i for i, r in enumerate(a.block_inds)}
    ib = {tuple(r): j for j, r in enumerate(b.block_inds)}
    both = [(ia[k], ib[k]) for k in ia if k in ib]
    only_a = [ia[k] for k in ia if k not in ib]
    only_b = [ib[k] for k in ib if k not in ia]
    return both, only_a, only_b


def linear_combination(bb, alpha: float, a: AbelianTensor, beta: float, b: AbelianTensor) -> AbelianTensor:
    """alpha*a + beta*b (abelian.cpp:2254-2302): blocks present in both go through ONE axpby launch,
    blocks present in only one of them are scaled copies (one more launch per side, if any)."""
    both, only_a, only_b = _align(a, b)
    rows, blocks = [], []
    if both:
        outs = bb.linear_combination_many(alpha, [a.blocks[i] for i, _ in both], beta, [b.blocks[j] for _, j in both])
        rows += [a.block_inds[i] for i, _ in both]
        blocks += outs
    if only_a:
        rows += [a.block_inds[i] for i in only_a]
        blocks += bb.mul_many(alpha, [a.blocks[i] for i in only_a])
    if only_b:
        rows += [b.block_inds[j] for j in only_b]
        blocks += bb.mul_many(beta, [b.blocks[j] for j in only_b])
    bi = np.array(rows, dtype=np.int64).reshape(len(rows), a.nlegs)
    return AbelianTensor(a.symmetry, a.legs, blocks, bi, a.num_codomain).sorted()


def scale(bb, alpha: float, a: AbelianTensor) -> AbelianTensor:
    """alpha * a, one launch over the block list (abelian.cpp:2230-2252)."""
    return AbelianTensor(a.symmetry, a.legs, bb.mul_many(alpha, a.blocks), a.block_inds, a.num_codomain)


def tdot(bb, a: AbelianTensor, b: AbelianTensor, legs_a: Sequence[int], legs_b: Sequence[int]) -> AbelianTensor:
    """``cyten.tdot(a, b, legs_a, legs_b)`` (tensors.py / abelian.cpp:1239-1469 behind it): contract leg
    ``legs_a[i]`` of a with leg ``legs_b[i]`` of b; the result carries a's remaining legs followed by b's
    remaining legs, each in their original order.  = two leg permutations (views) + one ``compose``."""
    legs_a = [int(i) % a.nlegs for i in legs_a]
    legs_b = [int(i) % b.nlegs for i in legs_b]
    if len(legs_a) != len(legs_b) or len(set(legs_a)) != len(legs_a) or len(set(legs_b)) != len(legs_b):
        raise ValueError('tdot: legs_a and legs_b must list the same number of distinct legs')
    keep_a = [i for i in range(a.nlegs) if i not in legs_a]
    keep_b = [i for i in range(b.nlegs) if i not in legs_b]
    # compose pairs a.legs[-1 - i] with b.legs[i]: a's contracted legs go last in REVERSED order
    a_p = permute_legs(bb, a, keep_a + legs_a[::-1])
    b_p = permute_legs(bb, b, legs_b + keep_b)
    return compose(bb, a_p, b_p, len(legs_a))


# ---------------------------------------------------------------------------------------------
# the remaining AbelianBackend callers of SURVEY.md section 8 row a10
# ---------------------------------------------------------------------------------------------

def _take_legs(bb, t: AbelianTensor, perm, num_codomain=None) -> AbelianTensor:
    """legs / block_inds columns / block axes in the order `perm`, rows NOT re-sorted (``block_inds.take_columns`` +
    ``permute_axes`` per block + ``make_data(..., is_sorted=false)`` of abelian.cpp:2883-2887 -- whose make_data sorts)."""
    perm = [int(p) for p in perm]
    blocks = [bb.permute_axes(b, perm) for b in t.blocks]
    bi = t.block_inds[:, perm] if len(blocks) else t.block_inds.reshape(0, len(perm))
    return AbelianTensor(t.symmetry, [t.legs[p] for p in perm], blocks, bi,
                         t.num_codomain if num_codomain is None else num_codomain).sorted()


def partial_compose(bb, a: AbelianTensor, b: AbelianTensor, a_first_leg: int) -> AbelianTensor:
    """``AbelianBackend::partial_compose`` (abelian.cpp:2853-2951): contract ALL domain legs of `b` (if `a_first_leg` lies
    in a's codomain; all codomain legs of b otherwise) with the consecutive legs of `a` that start at flat index
    `a_first_leg`; b's remaining legs take their place.  Flat legs = codomain + reversed domain, as in the reference.
    Three leg rotations (views + re-sorted block tables) around ONE ``compose``, i.e. one grouped launch."""
    a_n_cod, a_n = a.num_codomain, a.nlegs
    b_n_cod, b_n = b.num_codomain, b.nlegs
    b_n_dom = b_n - b_n_cod
    if a_first_leg < a_n_cod:
        num_contr, num_add = b_n_dom, b_n_cod
        perm_b = list(range(b_n_cod, b_n)) + list(range(b_n_cod))
        b_p = _take_legs(bb, b, perm_b)
    else:
        num_contr, num_add = b_n_cod, b_n_dom
        b_p = b
    if a_first_leg < 0 or a_first_leg + num_contr > a_n:
        raise ValueError('partial_compose: the contracted legs do not fit into a')
    perm_a = list(range(a_first_leg)) + list(range(a_first_leg + num_contr, a_n)) + list(range(a_first_leg, a_first_leg + num_contr))
    a_p = _take_legs(bb, a, perm_a)
    res = compose(bb, a_p, b_p, num_contr)
    n_keep = a_n - num_contr
    perm_res = list(range(a_first_leg)) + list(range(n_keep, n_keep + num_add)) + list(range(a_first_leg, n_keep))
    n_cod = a_n_cod - num_contr + num_add if a_first_leg < a_n_cod else a_n_cod
    return _take_legs(bb, res, perm_res, n_cod)


@dataclass
class Mask:
    """A projection from `large_leg` onto the kept basis states (cyten ``Mask``; AbelianBackendData with boolean 1-D blocks,
    abelian.cpp:2584-2680).  ``blocks[i]``: boolean numpy vector over the multiplicity of sector ``block_inds[i, 1]`` of the
    large leg (all-false sectors have no block); ``block_inds[i, 0]``: the sector's index on the small leg.  Masks are host
    data: their only use on the path is as gather / scatter index tables."""
    large_leg: Leg
    small_leg: Leg
    blocks: list
    block_inds: np.ndarray
    # device masks (``diagonal_to_mask``, ``mask_binary``, ``mask_unary``): `blocks` are boolean DEVICE blocks and
    # ``tables[i]`` holds the ascending kept positions of block i in device memory (what ``seg_compact_many`` returns), so
    # that ``mask_contract`` uploads nothing.  ``is_projection=False``: the dagger / transpose, an inclusion of the small leg
    # into the large one, whose ``block_inds`` columns are (large, small).
    tables: list | None = None
    is_projection: bool = True

    @property
    def large_col(self) -> int:
        """the column of ``block_inds`` that indexes the sectors of the large leg"""
        return 1 if self.is_projection else 0

    @classmethod
    def from_flags(cls, large_leg: Leg, flags) -> 'Mask':
        """from one boolean vector over the whole large leg (``mask_from_block``, abelian.cpp:2584-2640)"""
        flags = np.asarray(flags, dtype=bool)
        if flags.shape != (large_leg.dim,):
            raise ValueError('mask length does not match the leg')
        blocks, rows, sectors, mults = [], [], [], []
        for i in range(large_leg.nsec):
            m = flags[int(large_leg.slices[i]):int(large_leg.slices[i + 1])]
            if m.any():
                rows.append((len(sectors), i))
                blocks.append(m.copy())
                sectors.append(large_leg.sectors[i])
                mults.append(int(m.sum()))
        small = Leg(large_leg.symmetry, np.array(sectors, dtype=np.int64).reshape(len(mults), large_leg.symmetry.n), mults, large_leg.sign)
        return cls(large_leg, small, blocks, np.array(rows, dtype=np.int64).reshape(len(rows), 2))


def mask_contract(bb, t: AbelianTensor, mask: Mask, leg_idx: int, large_leg: bool = True) -> AbelianTensor:
    """``AbelianBackend::_mask_contract`` (abelian.cpp:2484-2583).  ``large_leg=True``: project leg `leg_idx` of `t` (the
    mask's large leg) onto the kept states, blocks of sectors without a kept state are dropped; ``False``: embed leg
    `leg_idx` (the small leg) into the large one, zeros elsewhere.  The reference loops ``apply_mask`` / ``enlarge_leg``
    over the common blocks; here the block table is matched on the host and ALL blocks go through one batched gather
    (``mask_gather_many``) or one zero fill + one batched scatter (``enlarge_leg_many``).  A device mask hands its
    position tables over as they are (``mask.tables``): no upload of index tables in either direction."""
    items, rows, legs = _mask_contract_items(t, mask, leg_idx, large_leg)
    if not items:
        return AbelianTensor(t.symmetry, legs, [], np.zeros((0, t.nlegs), np.int64), t.num_codomain)
    blocks = bb.mask_gather_many(items) if large_leg else bb.enlarge_leg_many(items)
    return AbelianTensor(t.symmetry, legs, blocks, np.array(rows, dtype=np.int64), t.num_codomain).sorted()


def _mask_contract_items(t: AbelianTensor, mask: Mask, leg_idx: int, large_leg: bool):
    """the host side of :func:`mask_contract`: (items for ``mask_gather_many`` / ``enlarge_leg_many``, rows of the new
    block table in the order of the items, new legs)"""
    leg_idx = int(leg_idx) % t.nlegs
    old_leg = t.legs[leg_idx]
    src_leg, dst_leg = (mask.large_leg, mask.small_leg) if large_leg else (mask.small_leg, mask.large_leg)
    if old_leg.nsec != src_leg.nsec or not np.array_equal(old_leg.sectors, src_leg.sectors) or not np.array_equal(old_leg.mults, src_leg.mults):
        raise ValueError('mask_contract: the leg of the tensor is not the leg of the mask')
    src_col = mask.large_col if large_leg else 1 - mask.large_col
    by_sector = {int(r[src_col]): j for j, r in enumerate(mask.block_inds)}
    # (the reference lexsorts by the contracted column and merges the two sorted columns; the result is sorted afterwards)
    items, rows = [], []
    for blk, row in zip(t.blocks, t.block_inds):
        j = by_sector.get(int(row[leg_idx]))
        if j is None:
            continue
        new_row = row.copy()
        new_row[leg_idx] = mask.block_inds[j, 1 - src_col]
        rows.append(new_row)
        if mask.tables is None:
            which = mask.blocks[j]
        elif large_leg:
            which = mask.tables[j]
        else:
            which = (mask.tables[j], int(mask.large_leg.mults[int(mask.block_inds[j, mask.large_col])]))
        items.append((blk, which, leg_idx))
    legs = list(t.legs)
    legs[leg_idx] = Leg(dst_leg.symmetry, dst_leg.sectors, dst_leg.mults, old_leg.sign)
    return items, rows, legs


def _common_sectors(cod: Leg, dom: Leg):
    """(j, k) of the sectors both legs hold, ascending (``iter_common_sorted_arrays`` on two sorted sector lists)"""
    where = {tuple(sec): k for k, sec in enumerate(dom.sectors.tolist())}
    return [(j, where[tuple(sec)]) for j, sec in enumerate(cod.sectors.tolist()) if tuple(sec) in where]


def _two_leg_decomposition(bb, t: AbelianTensor, new_mults, lq_mode: bool):
    """Shared body of ``AbelianBackend::qr`` (abelian.cpp:3084-3151) and ``::lq`` (:2304-2385) for a tensor with ONE
    codomain and ONE domain leg: every sector both legs hold gets an isometry block -- from the factorisation where `t`
    has a block (one batched call for all of them), a slice of the identity where it has none (then the triangular factor
    is zero and not stored)."""
    if t.nlegs != 2 or t.num_codomain != 1:
        raise ValueError('qr / lq of a tensor work on one codomain and one domain leg (combine the legs first)')
    cod, dom = t.legs
    common = _common_sectors(cod, dom)
    have = {(int(r[0]), int(r[1])): i for i, r in enumerate(t.block_inds)}
    sectors = np.array([cod.sectors[j] for j, _ in common], dtype=np.int64).reshape(len(common), t.symmetry.n)
    if new_mults is None:
        new_mults = [min(int(cod.mults[j]), int(dom.mults[k])) for j, k in common]
    if len(new_mults) != len(common):
        raise ValueError('new leg: one multiplicity per common sector')
    present = [(n, j, k) for n, (j, k) in enumerate(common) if (j, k) in have]
    srcs = [t.blocks[have[(j, k)]] for _, j, k in present]
    facs = (bb.matrix_lq_batched(srcs, False) if lq_mode else bb.matrix_qr_batched(srcs, False)) if srcs else []
    iso_blocks, iso_rows, tri_blocks, tri_rows = [], [], [], []
    it = iter(facs)
    done = {n for n, _, _ in present}
    for n, (j, k) in enumerate(common):
        if n in done:
            f0, f1 = next(it)
            tri, iso = (f0, f1) if lq_mode else (f1, f0)
            if iso.shape[0 if lq_mode else 1] != int(new_mults[n]):
                raise ValueError('new leg: multiplicity does not match the economic factorisation')
            tri_blocks.append(tri)
            tri_rows.append((j, n) if lq_mode else (n, k))
        else:
            dim = int(dom.mults[k] if lq_mode else cod.mults[j])
            eye = bb.eye_matrix(dim, dtype=srcs[0].dtype if srcs else None)
            nl = int(new_mults[n])
            iso = bb.get_item(eye, (slice(0, nl), slice(None)) if lq_mode else (slice(None), slice(0, nl)))
        iso_blocks.append(iso)
        iso_rows.append((n, k) if lq_mode else (j, n))
    new_in = Leg(t.symmetry, sectors, new_mults, +1)     # the new leg as a codomain-like leg ...
    new_out = Leg(t.symmetry, sectors, new_mults, -1)    # ... and as a domain-like one
    if lq_mode:
        L = AbelianTensor(t.symmetry, [cod, new_out], tri_blocks, np.array(tri_rows, dtype=np.int64).reshape(len(tri_rows), 2), 1).sorted()
        Q = AbelianTensor(t.symmetry, [new_in, dom], iso_blocks, np.array(iso_rows, dtype=np.int64).reshape(len(iso_rows), 2), 1).sorted()
        return L, Q
    Q = AbelianTensor(t.symmetry, [cod, new_out], iso_blocks, np.array(iso_rows, dtype=np.int64).reshape(len(iso_rows), 2), 1).sorted()
    R = AbelianTensor(t.symmetry, [new_in, dom], tri_blocks, np.array(tri_rows, dtype=np.int64).reshape(len(tri_rows), 2), 1).sorted()
    return Q, R


def qr_tensor(bb, t: AbelianTensor, new_mults=None):
    """``AbelianBackend::qr`` (abelian.cpp:3084-3151): t = Q R for a two-leg tensor, Q an isometry onto the new leg (sectors:
    those both legs hold; multiplicities `new_mults`, default min(m_cod, m_dom) = economic mode)."""
    return _two_leg_decomposition(bb, t, new_mults, False)


def lq_tensor(bb, t: AbelianTensor, new_mults=None):
    """``AbelianBackend::lq`` (abelian.cpp:2304-2385): t = L Q, Q an isometry from the new leg."""
    return _two_leg_decomposition(bb, t, new_mults, True)


def to_block_backend(bb_new, t: AbelianTensor, bb_old=None, dtype=None) -> AbelianTensor:
    """``AbelianBackend::to_block_backend`` (abelian.cpp:908-922): the same tensor with its blocks held by `bb_new`
    (``as_block`` per block; blocks of another backend travel through host arrays), optionally in another dtype."""
    blocks = []
    for b in t.blocks:
        if not (hasattr(bb_new, 'is_correct_block_type') and bb_new.is_correct_block_type(b)):
            b = (bb_old.to_numpy(b) if bb_old is not None else np.asarray(b))
        b = bb_new.as_block(b)
        blocks.append(bb_new.to_dtype(b, dtype) if dtype is not None else b)
    return AbelianTensor(t.symmetry, list(t.legs), blocks, t.block_inds.copy(), t.num_codomain, list(t.labels))


def move_to_device(bb, t: AbelianTensor, device) -> AbelianTensor:
    """``AbelianBackend::move_to_device`` (abelian.cpp:924-934): ``as_block(block, device=...)`` per block; a backend serves
    ONE device (`as_device` canonicalises the name and refuses others), so blocks already there are returned as they are."""
    dev = bb.as_device(device)
    return AbelianTensor(t.symmetry, list(t.legs), [bb.as_block(b, device=dev) for b in t.blocks], t.block_inds.copy(),
                         t.num_codomain, list(t.labels))


# ---------------------------------------------------------------------------------------------
# adjoint, diagonal tensors, traces, dense conversion
# ---------------------------------------------------------------------------------------------

def _is_complex_block(b) -> bool:
    return np.dtype(getattr(b, 'dtype', np.float64)).kind == 'c'


def _is_bool_block(b) -> bool:
    return np.dtype(getattr(b, 'dtype', np.float64)).kind == 'b'


def conj(bb, t: AbelianTensor) -> AbelianTensor:
    """Complex conjugate in the same leg order: every leg becomes its dual (same sectors, opposite sign), so the charge
    rule holds for the same block table.  Real blocks are their own conjugate (no launch); the complex blocks of the tensor
    go through ONE conjugating batched copy."""
    blocks = list(t.blocks)
    todo = [i for i, b in enumerate(blocks) if _is_complex_block(b)]
    if todo:
        new = bb.empty_many([t.blocks[i].shape for i in todo], dtype='complex128')
        bb.copy_many([(d, t.blocks[i]) for d, i in zip(new, todo)], conj=True)
        for d, i in zip(new, todo):
            blocks[i] = d
    return AbelianTensor(t.symmetry, [l.dual() for l in t.legs], blocks, t.block_inds.copy(), t.num_codomain, list(t.labels))


def dagger(bb, t: AbelianTensor) -> AbelianTensor:
    """``AbelianBackend::dagger`` (abelian.cpp:694-703): conjugate, reverse the flat legs (codomain and domain change
    places) and the columns of the block table, re-sort.  The axis reversal of the blocks is a view."""
    c = conj(bb, t)
    n = t.nlegs
    rev = list(range(n - 1, -1, -1))
    blocks = [bb.permute_axes(b, rev) for b in c.blocks]
    bi = c.block_inds[:, ::-1] if len(blocks) else c.block_inds.reshape(0, n)
    return AbelianTensor(t.symmetry, c.legs[::-1], blocks, bi, n - t.num_codomain, list(t.labels)[::-1]).sorted()


@dataclass
class DiagonalTensor:
    """cyten ``DiagonalTensor`` data: the diagonal of an operator from `leg` to itself, one 1-D block per sector that has
    one.  ``block_inds``: the sorted sector indices of the blocks (the reference stores the two equal columns
    ``[i, i]``, abelian.cpp:1643-1644)."""
    symmetry: Symmetry
    leg: Leg
    blocks: list
    block_inds: np.ndarray
    dtype: np.dtype | None = None     # of the blocks; it matters for a tensor without blocks (abelian.cpp:1622-1626)

    def __post_init__(self):
        self.block_inds = np.asarray(self.block_inds, dtype=np.int64).reshape(len(self.blocks))
        if self.dtype is None:
            kinds = {np.dtype(getattr(b, 'dtype', np.float64)).kind for b in self.blocks}
            self.dtype = np.dtype(np.complex128 if 'c' in kinds else np.bool_ if kinds == {'b'} else np.float64)
        self.dtype = np.dtype(self.dtype)

    @classmethod
    def from_numpy(cls, bb, leg: Leg, values) -> 'DiagonalTensor':
        """``diagonal_from_block`` (abelian.cpp:1636-1652): the full diagonal cut into one block per sector of `leg`"""
        values = np.asarray(values)
        if values.shape != (leg.dim,):
            raise ValueError('diagonal length does not match the leg')
        blocks = [bb.as_block(values[int(leg.slices[i]):int(leg.slices[i + 1])]) for i in range(leg.nsec)]
        return cls(leg.symmetry, leg, blocks, np.arange(leg.nsec))

    def to_numpy(self, bb) -> np.ndarray:
        """the full diagonal, zeros in the sectors without a block"""
        cplx = any(_is_complex_block(b) for b in self.blocks)
        dtype = np.bool_ if self.blocks and all(_is_bool_block(b) for b in self.blocks) else np.complex128 if cplx else np.float64
        out = np.zeros(self.leg.dim, dtype=dtype)
        for blk, i in zip(self.blocks, self.block_inds):
            out[int(self.leg.slices[i]):int(self.leg.slices[i + 1])] = bb.to_numpy(blk)
        return out


_UNARY_NAMES = ('abs', 'sqrt', 'exp', 'log', 'neg', 'square', 'reciprocal')
_UNARY_PARAM_NAMES = ('cutoff_inverse', 'stable_log', 'pow')


def diagonal_unary(bb, d: DiagonalTensor, func: str, param=None, maps_zero_to_zero: bool = True) -> DiagonalTensor:
    """``AbelianBackend::diagonal_elementwise_unary`` (abelian.cpp:743-782) for the elementwise functions the device
    serves by name: abs, sqrt, exp, log, neg, square, reciprocal, and -- with `param` -- cutoff_inverse (the pseudo-inverse of
    singular values), stable_log, pow.  The whole diagonal is ONE launch (``bb.unary_many``).  With
    ``maps_zero_to_zero=False`` the sectors without a block first get a zero block, as in the reference (:759-773)."""
    if func not in _UNARY_NAMES + _UNARY_PARAM_NAMES:
        raise ValueError(f'diagonal_unary: unknown function {func!r}')
    blocks, inds = list(d.blocks), d.block_inds
    if not maps_zero_to_zero:
        have = {int(i): b for i, b in zip(d.block_inds, d.blocks)}
        missing = [i for i in range(d.leg.nsec) if i not in have]
        for i, z in zip(missing, bb.zeros_many([(int(d.leg.mults[i]),) for i in missing]) if missing else []):
            have[i] = z
        inds = np.arange(d.leg.nsec)
        blocks = [have[i] for i in range(d.leg.nsec)]
    outs = bb.unary_many(blocks, func, param) if blocks else []
    return DiagonalTensor(d.symmetry, d.leg, list(outs), np.array(inds, dtype=np.int64))


def _same_space(a: Leg, b: Leg) -> bool:
    return a.nsec == b.nsec and np.array_equal(a.sectors, b.sectors) and np.array_equal(a.mults, b.mults)


def scale_axis(bb, t: AbelianTensor, d: DiagonalTensor, leg: int) -> AbelianTensor:
    """``AbelianBackend::scale_axis`` (abelian.cpp:3178-3232): multiply leg `leg` of `t` by the diagonal `d`.  Blocks of
    `t` whose sector on that leg has no block in `d` multiply to zero and are dropped (:3181-3182); the others go through
    ONE ``scale_axis_many`` launch instead of one ``scale_axis`` per block (:3223).  `d` is real."""
    leg = int(leg) % t.nlegs
    if t.symmetry != d.symmetry or not _same_space(t.legs[leg], d.leg):
        raise ValueError('scale_axis: the leg of the diagonal does not have the sectors and multiplicities of the leg of the tensor')
    if any(_is_complex_block(b) for b in d.blocks):
        raise NotImplementedError('scale_axis with a complex diagonal is not on the device path yet')
    by_sector = {int(i): b for i, b in zip(d.block_inds, d.blocks)}
    keep = [r for r, row in enumerate(t.block_inds) if int(row[leg]) in by_sector]
    blocks = bb.scale_axis_many([(t.blocks[r], by_sector[int(t.block_inds[r, leg])], leg) for r in keep]) if keep else []
    return AbelianTensor(t.symmetry, list(t.legs), list(blocks), t.block_inds[keep].reshape(len(keep), t.nlegs), t.num_codomain,
                         list(t.labels))


def dual_sector_map(symmetry: Symmetry, a: Leg, b: Leg):
    """For every sector index of `a` the index of the sector of `b` whose charge cancels it (``sign_a q_a + sign_b q_b = 0``
    under the moduli); None unless this is a bijection between the two sector lists that keeps the multiplicities -- i.e.
    unless the legs are dual to each other and can be traced."""
    if a.nsec != b.nsec:
        return None
    where = {tuple(q): k for k, q in enumerate(b.sectors.tolist())}
    want = symmetry.reduce(-a.sign * b.sign * a.sectors).reshape(a.nsec, symmetry.n)
    out = np.zeros(a.nsec, dtype=np.int64)
    for i, q in enumerate(want.tolist()):
        k = where.get(tuple(q))
        if k is None or int(a.mults[i]) != int(b.mults[k]):
            return None
        out[i] = k
    return out if len(set(out.tolist())) == a.nsec else None


def partial_trace(bb, t: AbelianTensor, pairs):
    """``AbelianBackend::partial_trace`` (abelian.cpp:2954-3081): trace leg ``i`` against leg ``j`` for every ``(i, j)`` of
    `pairs`.  A pair is traceable if the legs are dual to each other (:func:`dual_sector_map`); a block contributes if its
    charges cancel on every pair -- one rule for legs on opposite sides and on the same side (:2996-3014).  The remaining legs
    keep their order, ``num_codomain`` counts those that were in the codomain, and blocks with the same remaining sector
    indices are summed.  ALL result blocks are computed by ONE ``trace_partial_grouped`` launch; the reference calls
    ``trace_partial`` per block and adds with ``operator+`` (:3016-3029).  With no remaining leg the result is a Python
    float / complex (the ``Scalar`` case, :3042-3055; 0 if no block is on the diagonal)."""
    n = t.nlegs
    pairs = [(int(i) % n, int(j) % n) for i, j in pairs]
    traced = [k for p in pairs for k in p]
    if len(set(traced)) != len(traced):
        raise ValueError('partial_trace: a leg is listed twice')
    maps = []
    for i, j in pairs:
        m = dual_sector_map(t.symmetry, t.legs[i], t.legs[j])
        if m is None:
            raise ValueError(f'partial_trace: legs {i} and {j} are not dual to each other')
        maps.append(m)
    idcs1, idcs2 = [i for i, _ in pairs], [j for _, j in pairs]
    remaining = [k for k in range(n) if k not in traced]
    bi = t.block_inds
    on_diag = np.ones(len(t.blocks), dtype=bool)
    for (i, j), m in zip(pairs, maps):
        on_diag &= m[bi[:, i]] == bi[:, j]
    groups: dict = {}
    for r in np.flatnonzero(on_diag).tolist():    # ascending block index: the summation order of every result block
        groups.setdefault(tuple(bi[r, remaining].tolist()), []).append(r)
    legs = [t.legs[k] for k in remaining]
    if not remaining:
        if not groups:
            return 0.0
        blk = bb.trace_partial_grouped([((), [(t.blocks[r], idcs1, idcs2, []) for r in groups[()]])])[0]
        return np.asarray(bb.to_numpy(blk)).reshape(()).item()
    rows = np.array(list(groups.keys()), dtype=np.int64).reshape(len(groups), len(remaining))
    order = _lexsort_rows(rows)
    rows = rows[order]
    members = [groups[tuple(r)] for r in rows.tolist()]
    outputs = [(tuple(int(l.mults[s]) for l, s in zip(legs, row)), [(t.blocks[r], idcs1, idcs2, remaining) for r in mem])
               for row, mem in zip(rows.tolist(), members)]
    blocks = bb.trace_partial_grouped(outputs) if outputs else []
    labels = [t.labels[k] for k in remaining] if len(t.labels) == n else []
    return AbelianTensor(t.symmetry, legs, list(blocks), rows, sum(1 for k in remaining if k < t.num_codomain), labels)


def trace_full(bb, t: AbelianTensor):
    """``AbelianBackend::trace_full`` (abelian.cpp:3595-3620): leg ``c`` against leg ``nlegs - 1 - c`` (codomain against
    domain), through :func:`partial_trace` -- one launch, one number back."""
    if t.nlegs % 2:
        raise ValueError('trace_full: the tensor needs as many domain as codomain legs')
    return partial_trace(bb, t, [(c, t.nlegs - 1 - c) for c in range(t.nlegs // 2)])


def _block_slices(legs, row):
    return tuple(slice(int(l.slices[i]), int(l.slices[i + 1])) for l, i in zip(legs, row))


def to_dense_block(bb, t: AbelianTensor):
    """``AbelianBackend::to_dense_block`` (abelian.cpp:3571-3592): ONE zero-filled block of the full shape, all blocks
    placed by ONE batched copy (the reference assigns ``res[slices] = block`` per block)."""
    cplx = any(_is_complex_block(b) for b in t.blocks)
    dense = bb.zeros_many([tuple(l.dim for l in t.legs)], dtype='complex128' if cplx else None)[0]
    pairs = []
    for blk, row in zip(t.blocks, t.block_inds):
        if cplx and not _is_complex_block(blk):
            blk = bb.as_complex(blk)
        pairs.append((bb.get_item(dense, _block_slices(t.legs, row)), blk))
    if pairs:
        bb.copy_many(pairs)
    return dense


def from_dense_block(bb, symmetry: Symmetry, legs, block, num_codomain: int = 0, tol=1e-6) -> AbelianTensor:
    """``AbelianBackend::from_dense_block`` (abelian.cpp:1829-1858): every charge-allowed block (zero ones included) is cut
    out of the dense `block` by ONE batched copy.  With a `tol` (default: that of symmetric_tensor.h:76) the part of
    `block` outside the allowed blocks must be small, ``norm(block - projected) <= tol * norm(block)`` -- both norms are
    reductions on the device -- else ``ValueError('Block is not symmetric up to tolerance.')``."""
    legs = list(legs)
    if tuple(block.shape) != tuple(l.dim for l in legs):
        raise ValueError('from_dense_block: the block does not have the shape of the legs')
    inds = AbelianTensor.allowed_block_inds(symmetry, legs)
    cplx = _is_complex_block(block)
    views = [bb.get_item(block, _block_slices(legs, row)) for row in inds]
    blocks = bb.empty_many([v.shape for v in views], dtype='complex128' if cplx else None) if views else []
    if views:
        bb.copy_many(list(zip(blocks, views)))
    res = AbelianTensor(symmetry, legs, list(blocks), inds, num_codomain)
    if tol is not None:
        projected = to_dense_block(bb, res)
        diff = bb.linear_combination_many(1.0, [block], -1.0, [projected])
        if bb.norm_many(diff) > tol * bb.norm_many([block]):
            raise ValueError('Block is not symmetric up to tolerance.')
    return res


# ---------------------------------------------------------------------------------------------
# leg pipes: combine_legs / split_legs
# ---------------------------------------------------------------------------------------------

CYB_MAX_NDIM = 8    # most axes a strided copy of the library takes (include/cyten_amd.h)


_PIPE_CACHE: dict = {}


class LegPipe(Leg):
    """``AbelianLegPipe`` mirror: the product of k >= 1 legs seen as ONE leg (build it with :meth:`from_legs`).

    Sector ``Q`` of the pipe satisfies ``sign * Q = sum_k sign_k * q_k`` under the moduli; sectors are sorted as `Leg` sorts
    them and the multiplicity of ``Q`` is the sum of ``prod_k mult`` over the sector combinations that fuse to it.

    * ``block_ind_map``: int64, one row ``[start, stop, i_1 .. i_k, J]`` per sector combination, sorted by ``J``; within a ``J``
      in C order of ``(i_1 .. i_k)`` (last leg fastest) for ``cstyle=True``, in F order (first leg fastest) otherwise.
      ``start:stop`` is the slice of sector ``J`` the combination occupies; inside it the basis states run in the same style
      over the constituents' multiplicities.  ``block_ind_map_slices[J]:block_ind_map_slices[J + 1]`` are the rows of ``J``.
    * ``basis_perm``: int64 of length ``dim``; entry ``j`` is the flat C index, in the dense product of the constituent legs,
      of basis state ``j`` of the pipe -- the dense statement of what the pipe is.

    The reference decides the internal order of a pipe by ``combine_cstyle != in_domain`` because its flat leg list reverses
    the domain; this mirror does not reverse domain legs, so the style of a pipe is its ``cstyle`` wherever it stands, and
    :meth:`dual` keeps it (no style flip)."""

    def __init__(self, symmetry, sectors, mults, sign, legs, cstyle, block_ind_map, block_ind_map_slices):
        super().__init__(symmetry, sectors, mults, sign)     # (sectors arrive sorted: the order is kept)
        self.legs = list(legs)
        self.cstyle = bool(cstyle)
        self.block_ind_map = block_ind_map
        self.block_ind_map_slices = block_ind_map_slices
        self._shared = {}

    @classmethod
    def from_legs(cls, symmetry: Symmetry, legs, sign: int = +1, cstyle: bool = True) -> 'LegPipe':
        legs = list(legs)
        if not legs:
            raise ValueError('LegPipe: at least one leg')
        sign = int(sign)
        if sign not in (+1, -1):
            raise ValueError('LegPipe: sign must be +1 or -1')
        k = len(legs)
        # the tables depend on the content of the constituents only: built once, shared by every pipe of that content
        # (callers must not modify them); the pipe object itself is new, so that it holds the legs it was given
        key = (_legs_key(symmetry, legs, [l.sign for l in legs]), sign, bool(cstyle))
        hit = _PIPE_CACHE.get(key)
        if hit is None:
            # C order of the reversed legs is F order of the legs: fuse the reversed list and turn the index tuples back
            walk = legs if cstyle else legs[::-1]
            fmap = _fused_sector_maps(symmetry, walk, [sign * l.sign for l in walk])
            charges = sorted(fmap.keys(), key=lambda c: tuple(reversed(c)))
            rows, slices, mults = [], [0], []
            for J, ch in enumerate(charges):
                for idx, off, sz in fmap[ch]:
                    rows.append((off, off + sz) + (idx if cstyle else idx[::-1]) + (J,))
                slices.append(len(rows))
                mults.append(fmap[ch][-1][1] + fmap[ch][-1][2])
            bim = np.array(rows, dtype=np.int64).reshape(len(rows), k + 3)
            sectors = np.array(charges, dtype=np.int64).reshape(len(charges), symmetry.n)
            hit = _cache_put(_PIPE_CACHE, key, (sectors, np.array(mults, dtype=np.int64), bim, np.array(slices, dtype=np.int64), {}))
        sectors, mults, bim, slices, shared = hit
        pipe = cls(symmetry, sectors, mults, sign, legs, cstyle, bim, slices)
        pipe._shared = shared        # (lazily built `where` / `basis_perm` of this content)
        return pipe

    @property
    def num_legs(self):
        return len(self.legs)

    def where(self) -> dict:
        """{(i_1 .. i_k): (J, start, stop)}"""
        out = self._shared.get('where')
        if out is None:
            out = self._shared['where'] = {tuple(r[2:-1]): (r[-1], r[0], r[1]) for r in self.block_ind_map.tolist()}
        return out

    @property
    def basis_perm(self) -> np.ndarray:
        if self._shared.get('basis_perm') is None:
            dims = [l.dim for l in self.legs]
            dense_strides = [int(np.prod(dims[i + 1:], dtype=np.int64)) for i in range(len(dims))]
            out = np.zeros(self.dim, dtype=np.int64)
            for r in self.block_ind_map.tolist():
                start, stop, idx, J = r[0], r[1], r[2:-1], r[-1]
                flat = np.zeros((), dtype=np.int64)
                for l, i, ds in zip(self.legs, idx, dense_strides):
                    flat = flat[..., None] + ds * np.arange(int(l.slices[i]), int(l.slices[i + 1]), dtype=np.int64)
                base = int(self.slices[J])
                out[base + start:base + stop] = flat.reshape(-1) if self.cstyle else flat.T.reshape(-1)
            self._shared['basis_perm'] = out
        return self._shared['basis_perm']

    def dual(self) -> 'LegPipe':
        """The pipe of the dual legs with the opposite sign: the same sectors, multiplicities, internal order and style."""
        return LegPipe.from_legs(self.symmetry, [l.dual() for l in self.legs], -self.sign, self.cstyle)

    def can_contract_with(self, other: 'Leg') -> bool:
        """The base rule; against another pipe also pairwise contractible constituents and the same style (two pipes with
        equal sectors but another internal order would otherwise contract silently wrong)."""
        if not Leg.can_contract_with(self, other):
            return False
        if isinstance(other, LegPipe):
            return (self.cstyle == other.cstyle and len(self.legs) == len(other.legs)
                    and all(a.can_contract_with(b) for a, b in zip(self.legs, other.legs)))
        return True

    def __repr__(self):
        return f'LegPipe({len(self.legs)} legs, nsec={self.nsec}, dim={self.dim}, sign={self.sign:+d}, {"C" if self.cstyle else "F"})'


def _same_leg(a: Leg, b: Leg) -> bool:
    return a.sign == b.sign and _same_space(a, b)


def _sub_strides(stride: int, mults, cstyle: bool):
    """strides of the constituent axes a slice of a pipe axis (element stride `stride`) splits into"""
    out, acc = [0] * len(mults), int(stride)
    for k in (range(len(mults) - 1, -1, -1) if cstyle else range(len(mults))):
        out[k] = acc
        acc *= int(mults[k])
    return out


def _c_strides_of(shape):
    out, acc = [0] * len(shape), 1
    for k in range(len(shape) - 1, -1, -1):
        out[k] = acc
        acc *= int(shape[k])
    return out


def _place_records(n):
    from . import _lib
    return np.zeros(n, dtype=_lib.PLACE_DTYPE)


def _block_strides(bb, blocks):
    """element strides of device blocks (None for the blocks of a backend without placement plans)"""
    return tuple(tuple(b.strides) for b in blocks) if _has_plans(bb) else None


def _has_plans(bb) -> bool:
    return getattr(bb, 'place_plan', None) is not None


_COMBINE_CACHE: dict = {}
_SPLIT_CACHE: dict = {}


def _promote_mixed(bb, blocks):
    """(blocks, is complex): a list mixing float64 and complex128 blocks is promoted to complex128 first"""
    # (device blocks answer `is_complex` from their buffer; the dtype property behind _is_complex_block costs more per block)
    kinds = [b.is_complex for b in blocks] if blocks and hasattr(blocks[0], 'is_complex') else [_is_complex_block(b) for b in blocks]
    if any(kinds) and not all(kinds):
        if hasattr(bb, 'as_complex_many'):
            blocks = bb.as_complex_many(blocks)
        else:
            blocks = [b if c else bb.as_complex(b) for b, c in zip(blocks, kinds)]
    return list(blocks), any(kinds)


def combine_legs(bb, t: AbelianTensor, groups, pipes=None, signs=None, cstyle=True, num_codomain=None) -> AbelianTensor:
    """``AbelianBackend::combine_legs`` (abelian.cpp:1022-1219) behind the tensor level's leg permutation: every group of
    `groups` (disjoint lists of leg indices, in any order, not necessarily adjacent) becomes ONE :class:`LegPipe`, standing
    where the first-listed leg of the group stood among the legs that remain; the other legs keep their relative order.

    `pipes`: ready-made pipes (checked against the legs), else they are built with `signs` (default +1 each) and `cstyle`
    (one flag, or one per group).  Labels become ``'(a.b)'``; ``num_codomain`` defaults to the number of result legs whose
    first constituent lay in the codomain.  All old blocks that land in one new block are embedded in it, zeros elsewhere;
    the result is lexsorted.

    The permutation is no separate pass: each old block is read through its (possibly permuted) strides by the SAME launch
    that writes it to its place.  With a backend that offers ``place_plan`` the records of the structure -- legs, groups,
    block table, element size, source strides -- become a device-resident plan once (cached by content) and a call uploads
    the two address tables only; the zero fill is skipped when the old blocks cover the result.  Other backends take
    ``zeros_many`` + one ``copy_many``."""
    n = t.nlegs
    if n > CYB_MAX_NDIM:
        raise ValueError(f'combine_legs: tensors of more than {CYB_MAX_NDIM} legs are not supported')
    groups = [[int(i) % n for i in g] for g in groups]
    flat = [i for g in groups for i in g]
    if any(len(g) == 0 for g in groups):
        raise ValueError('combine_legs: empty group')
    if len(set(flat)) != len(flat):
        raise ValueError('combine_legs: the groups overlap')
    ng = len(groups)
    styles = [bool(cstyle)] * ng if isinstance(cstyle, (bool, int)) else [bool(c) for c in cstyle]
    signs = [+1] * ng if signs is None else [int(s) for s in signs]
    if len(styles) != ng or len(signs) != ng or (pipes is not None and len(pipes) != ng):
        raise ValueError('combine_legs: one pipe / sign / style per group')
    sym = t.symmetry
    if pipes is None:
        pipes = [LegPipe.from_legs(sym, [t.legs[i] for i in g], sg, cs) for g, sg, cs in zip(groups, signs, styles)]
    else:
        pipes = list(pipes)
        for g, p in zip(groups, pipes):
            if not isinstance(p, LegPipe) or len(p.legs) != len(g) or not all(_same_leg(a, t.legs[i]) for a, i in zip(p.legs, g)):
                raise ValueError('combine_legs: a pipe does not consist of the legs of its group')
    # ---- result legs: (group number | None, source legs) in result order
    first = {g[0]: k for k, g in enumerate(groups)}
    grouped = set(flat)
    res = []
    for i in range(n):
        if i in first:
            res.append((first[i], groups[first[i]]))
        elif i not in grouped:
            res.append((None, [i]))
    legs = [t.legs[src[0]] if g is None else pipes[g] for g, src in res]
    labels = []
    if len(t.labels) == n:
        labels = [t.labels[src[0]] if g is None else '(' + '.'.join(str(t.labels[i]) for i in src) + ')' for g, src in res]
    if num_codomain is None:
        num_codomain = sum(1 for _, src in res if src[0] < t.num_codomain)
    if len(t.blocks) == 0:
        return AbelianTensor(sym, legs, [], np.zeros((0, len(res)), np.int64), num_codomain, labels)
    blocks, cplx = _promote_mixed(bb, t.blocks)
    esz = 16 if cplx else 8
    native = _has_plans(bb)
    binds = np.ascontiguousarray(t.block_inds, dtype=np.int64)
    key = (_legs_key(sym, t.legs, [l.sign for l in t.legs]), tuple(map(tuple, groups)), tuple((p.sign, p.cstyle) for p in pipes),
           binds.shape, binds.tobytes(), esz, _block_strides(bb, blocks))
    plan = _COMBINE_CACHE.get(key)
    if plan is None:
        plan = _cache_put(_COMBINE_CACHE, key, _combine_plan(t.legs, binds, res, pipes, legs,
                                                             [tuple(b.strides) for b in blocks] if native else None))
    new_rows, new_shapes = plan['rows'], plan['shapes']
    if native:
        if plan.get('native') is None:
            plan['native'] = bb.place_plan(plan['records'], len(blocks), len(new_shapes), esz)
        dt = 'complex128' if cplx else None
        new_blocks = bb.empty_many(new_shapes, dtype=dt) if plan['covers'] else bb.zeros_many(new_shapes, dtype=dt)
        # address tables from the blocks at hand (never from a cached table: block lists are mutable)
        bb.place_enqueue(plan['native'], [b.ptr for b in blocks], [b.ptr for b in new_blocks])
    else:
        new_blocks = bb.zeros_many(new_shapes, dtype='complex128' if cplx else None)
        pairs = []
        for blk, (dst, key_sl, perm, merged) in zip(blocks, plan['generic']):
            pairs.append((bb.get_item(new_blocks[dst], key_sl), bb.reshape(bb.permute_axes(blk, perm), merged)))
        bb.copy_many(pairs)
    return AbelianTensor(sym, legs, list(new_blocks), new_rows.copy(), num_codomain, labels)


def _combine_plan(old_legs, binds, res, pipes, legs, src_strides):
    """The placement of one combine_legs structure: result block table (lexsorted, no duplicates), result shapes, and per
    old block where it goes -- as placement records (`src_strides` given) and as (slices, axis order, merged shape) for
    the generic route."""
    nres = len(res)
    rows = np.zeros((len(binds), nres), dtype=np.int64)
    starts = np.zeros((len(binds), nres), dtype=np.int64)
    stops = np.zeros((len(binds), nres), dtype=np.int64)
    bl = binds.tolist()
    for r, (g, src) in enumerate(res):
        if g is None:
            rows[:, r] = binds[:, src[0]]
            stops[:, r] = old_legs[src[0]].mults[binds[:, src[0]]]
        else:
            where = pipes[g].where()
            for b, row in enumerate(bl):
                rows[b, r], starts[b, r], stops[b, r] = where[tuple(row[i] for i in src)]
    order = _lexsort_rows(rows)
    srt = rows[order]
    new_of = np.zeros(len(binds), dtype=np.int64)
    if len(srt):
        is_new = np.concatenate([[True], np.any(srt[1:] != srt[:-1], axis=1)])
        new_of[order] = np.cumsum(is_new) - 1
        new_rows = srt[is_new]
    else:
        new_rows = srt
    shapes = [tuple(int(l.mults[i]) for l, i in zip(legs, row)) for row in new_rows.tolist()]
    # axis order of the source: result order, the constituents of a pipe in the order the pipe lists them
    perm_c = [i for _, src in res for i in src]
    out = dict(rows=new_rows, shapes=shapes, generic=[], records=None, native=None)
    placed = 0
    recs = _place_records(len(binds)) if src_strides is not None else None
    for b, row in enumerate(bl):
        dst = int(new_of[b])
        dstr = _c_strides_of(shapes[dst])
        ext = [int(old_legs[i].mults[row[i]]) for i in range(len(row))]
        placed += math.prod(ext)
        # generic route: an F-style pipe reads its constituents in reversed axis order, so that a C-order reshape merges them
        perm_g, merged = [], []
        for r, (g, src) in enumerate(res):
            perm_g += src if (g is None or pipes[g].cstyle) else src[::-1]
            merged.append(int(stops[b, r] - starts[b, r]))
        key_sl = tuple(slice(int(starts[b, r]), int(stops[b, r])) for r in range(nres))
        out['generic'].append((dst, key_sl, perm_g, merged))
        if recs is not None:
            ds, off = [], 0
            for r, (g, src) in enumerate(res):
                off += int(starts[b, r]) * dstr[r]
                ds += [dstr[r]] if g is None else _sub_strides(dstr[r], [ext[i] for i in src], pipes[g].cstyle)
            nd = len(perm_c)
            rec = recs[b]
            rec['src_block'], rec['dst_block'], rec['ndim'], rec['dst_offset'] = b, dst, nd, off
            rec['shape'][:nd] = [ext[i] for i in perm_c]
            rec['src_strides'][:nd] = [src_strides[b][i] for i in perm_c]
            rec['dst_strides'][:nd] = ds
    out['records'] = recs
    out['covers'] = placed == sum(math.prod(sh) for sh in shapes)    # (distinct old blocks never overlap: equal sizes = all covered)
    return out


def _split_label(label, k):
    """the k labels inside ``'(a.b)'`` (dots inside nested brackets do not split), else ``label.0 .. label.k-1``"""
    s = str(label)
    if s.startswith('(') and s.endswith(')'):
        parts, depth, cur = [], 0, ''
        for ch in s[1:-1]:
            depth += ch == '('
            depth -= ch == ')'
            if ch == '.' and depth == 0:
                parts.append(cur)
                cur = ''
            else:
                cur += ch
        parts.append(cur)
        if len(parts) == k:
            return parts
    return [f'{s}.{j}' for j in range(k)]


def split_legs(bb, t: AbelianTensor, leg_idcs=None, contiguous: bool = False) -> AbelianTensor:
    """``AbelianBackend::split_legs`` (abelian.cpp:3235-3437), the inverse of :func:`combine_legs`: every leg of `leg_idcs`
    (default: all legs that are pipes; one level of nesting per call) is replaced by its constituents.  Every old block
    yields one new block per row of the pipe's ``block_ind_map`` inside its sector (for several split legs: per element of
    the product of the rows): the slice ``start:stop`` of that axis, reshaped into the constituent extents (reversed
    sub-axes for an F-style pipe).  Slicing and splitting an axis is always expressible in strides, so the new blocks are
    VIEWS of the old ones (no launch; the next ``compose`` makes contiguous what it needs).  ``contiguous=True`` gathers all
    new blocks into one pooled allocation with one placement-plan launch (``reverse``: the plan's records are those of the
    combination that would undo the split)."""
    n = t.nlegs
    if leg_idcs is None:
        leg_idcs = [i for i, l in enumerate(t.legs) if isinstance(l, LegPipe)]
    leg_idcs = sorted({int(i) % n for i in leg_idcs})
    for i in leg_idcs:
        if not isinstance(t.legs[i], LegPipe):
            raise ValueError('Not a LegPipe.')
    split = set(leg_idcs)
    legs, labels = [], []
    have_labels = len(t.labels) == n
    for i, l in enumerate(t.legs):
        legs += l.legs if i in split else [l]
        if have_labels:
            labels += _split_label(t.labels[i], len(l.legs)) if i in split else [t.labels[i]]
    if len(legs) > CYB_MAX_NDIM:
        raise ValueError(f'split_legs: tensors of more than {CYB_MAX_NDIM} legs are not supported')
    num_codomain = sum(len(t.legs[i].legs) if i in split else 1 for i in range(min(t.num_codomain, n)))
    sym = t.symmetry
    if len(t.blocks) == 0:
        return AbelianTensor(sym, legs, [], np.zeros((0, len(legs)), np.int64), num_codomain, labels)
    new_rows, views, origin = [], [], []     # origin: (old block, [(old axis, start, constituent extents, cstyle) ...])
    for b, (blk, row) in enumerate(zip(t.blocks, t.block_inds.tolist())):
        choices = []
        for i in leg_idcs:
            p = t.legs[i]
            lo, hi = int(p.block_ind_map_slices[row[i]]), int(p.block_ind_map_slices[row[i] + 1])
            choices.append(p.block_ind_map[lo:hi].tolist())
        for combo in itertools.product(*choices):
            key_sl, shape, perm, new_row, parts = [slice(None)] * n, [], [], [], []
            it = iter(combo)
            for i, l in enumerate(t.legs):
                if i not in split:
                    shape.append(int(l.mults[row[i]]))
                    perm.append(len(perm))
                    new_row.append(row[i])
                    continue
                m = next(it)
                idx = m[2:-1]
                ext = [int(c.mults[j]) for c, j in zip(l.legs, idx)]
                key_sl[i] = slice(m[0], m[1])
                k0 = len(perm)
                shape += ext if l.cstyle else ext[::-1]
                perm += list(range(k0, k0 + len(ext))) if l.cstyle else list(range(k0 + len(ext) - 1, k0 - 1, -1))
                new_row += idx
                parts.append((i, m[0], ext, l.cstyle))
            v = bb.reshape(bb.get_item(blk, tuple(key_sl)), shape)
            views.append(v if perm == sorted(perm) else bb.permute_axes(v, perm))
            new_rows.append(new_row)
            origin.append((b, parts))
    new_rows = np.array(new_rows, dtype=np.int64).reshape(len(views), len(legs))
    if contiguous and _has_plans(bb):
        views = _split_gather(bb, t, leg_idcs, [v.shape for v in views], origin)
    elif contiguous:
        views = bb.contiguous_many(views)
    return AbelianTensor(sym, legs, list(views), new_rows, num_codomain, labels).sorted()


def _split_gather(bb, t, leg_idcs, shapes, origin):
    """the new blocks of a split as C-contiguous blocks of ONE pool, gathered by one placement-plan launch in reverse"""
    blocks, cplx = _promote_mixed(bb, t.blocks)
    esz = 16 if cplx else 8
    binds = np.ascontiguousarray(t.block_inds, dtype=np.int64)
    key = (_legs_key(t.symmetry, t.legs, [l.sign for l in t.legs]),
           tuple((i, t.legs[i].cstyle, _legs_key(t.symmetry, t.legs[i].legs, [l.sign for l in t.legs[i].legs])) for i in leg_idcs),
           binds.shape, binds.tobytes(), esz, _block_strides(bb, blocks))
    plan = _SPLIT_CACHE.get(key)
    if plan is None:
        recs = _place_records(len(shapes))
        for j, (shape, (b, parts)) in enumerate(zip(shapes, origin)):
            old = blocks[b].strides
            by_axis = {i: (start, ext, cs) for i, start, ext, cs in parts}
            ds, off = [], 0
            for i in range(t.nlegs):
                if i in by_axis:
                    start, ext, cs = by_axis[i]
                    off += start * old[i]
                    ds += _sub_strides(old[i], ext, cs)
                else:
                    ds.append(old[i])
            nd = len(shape)
            rec = recs[j]
            rec['src_block'], rec['dst_block'], rec['ndim'], rec['dst_offset'] = j, b, nd, off
            rec['shape'][:nd] = shape
            rec['src_strides'][:nd] = _c_strides_of(shape)
            rec['dst_strides'][:nd] = ds
        plan = _cache_put(_SPLIT_CACHE, key, dict(native=bb.place_plan(recs, len(shapes), len(blocks), esz)))
    new_blocks = bb.empty_many(shapes, dtype='complex128' if cplx else None)
    bb.place_enqueue(plan['native'], [b.ptr for b in new_blocks], [b.ptr for b in blocks], reverse=True)
    return new_blocks


# ---------------------------------------------------------------------------------------------
# functions of a square tensor
# ---------------------------------------------------------------------------------------------

def _square_half(t: AbelianTensor, what: str) -> int:
    """k of a tensor of 2k legs that maps its first k legs to themselves: ``legs[n - 1 - i]`` contracts with ``legs[i]``,
    the pairing ``compose(t, t, k)`` uses"""
    n = t.nlegs
    if n == 0 or n % 2:
        raise ValueError(f'{what}: a tensor of {n} legs is not square (an even number of legs is required)')
    for i in range(n // 2):
        if not t.legs[n - 1 - i].can_contract_with(t.legs[i]):
            raise ValueError(f'{what}: leg {n - 1 - i} cannot be contracted with leg {i}')
    return n // 2


def _act_diagonal(bb, t: AbelianTensor, block_method_many, all_sectors: bool) -> AbelianTensor:
    if t.nlegs != 2 or not t.legs[1].can_contract_with(t.legs[0]):
        raise ValueError('act_block_diagonal_square_matrix: a two-leg tensor [leg, leg.dual()] is required')
    leg = t.legs[0]
    have = {}
    for (i, j), b in zip(t.block_inds.tolist(), t.blocks):
        if i != j:
            raise ValueError(f'act_block_diagonal_square_matrix: block ({i}, {j}) is not on the diagonal')
        have[i] = b
    sectors = list(range(leg.nsec)) if all_sectors else sorted(have)
    entries = [have[j] if j in have else (int(leg.mults[j]), None) for j in sectors]
    blocks = list(block_method_many(entries)) if entries else []
    if len(blocks) != len(entries):
        raise ValueError('act_block_diagonal_square_matrix: the block method must return one block per entry')
    return AbelianTensor(t.symmetry, list(t.legs), blocks, np.array([[j, j] for j in sectors], dtype=np.int64).reshape(len(sectors), 2),
                         t.num_codomain, list(t.labels))


def act_block_diagonal_square_matrix(bb, t: AbelianTensor, block_method_many, dtype_map=None) -> AbelianTensor:
    """``AbelianBackend::act_block_diagonal_square_matrix`` (abelian.cpp:562-593) for a two-leg tensor ``[leg, leg.dual()]``:
    a function of a block-diagonal matrix is that function of every diagonal block.  The result holds ALL ``leg.nsec``
    diagonal blocks -- a sector without a block is a zero block and f(0) need not vanish (:574-584) --, so
    ``block_inds == [[j, j] for j in range(nsec)]``.  Where the reference calls a block method once per sector,
    `block_method_many` receives the whole list once: the present blocks and ``(n, None)`` for the zero blocks, in sector
    order; it returns one block per entry.  `dtype_map` (the reference's map from the dtype of the tensor to that of the
    result, :566-569) is accepted for the same call shape; a tensor here has no dtype of its own: it is that of the blocks the
    method returns."""
    return _act_diagonal(bb, t, block_method_many, True)


def _on_square_matrix(bb, t: AbelianTensor, k: int, block_method_many, all_sectors: bool = True) -> AbelianTensor:
    """`t` as a two-leg tensor of pipes -> `_act_diagonal` -> split and permuted back.  The codomain ``0 .. k-1`` becomes a
    pipe and the REVERSED domain ``n-1 .. k`` its dual: the same sectors in the same internal order, so that every block is
    square with the same basis on its rows and columns."""
    n = t.nlegs
    if n == 2:
        return _act_diagonal(bb, t, block_method_many, all_sectors)
    pipe = LegPipe.from_legs(t.symmetry, t.legs[:k], +1)
    m = combine_legs(bb, t, [list(range(k)), list(range(n - 1, k - 1, -1))], pipes=[pipe, pipe.dual()], num_codomain=1)
    r = split_legs(bb, _act_diagonal(bb, m, block_method_many, all_sectors))
    r = permute_legs(bb, r, list(range(k)) + list(range(n - 1, k - 1, -1)))
    return AbelianTensor(t.symmetry, list(t.legs), r.blocks, r.block_inds, t.num_codomain, list(t.labels))


def exp(bb, t: AbelianTensor, factor=1.0) -> AbelianTensor:
    """``exp(factor * t)`` of a tensor of 2k legs that maps its first k legs to themselves (``legs[n-1-i]`` contracts with
    ``legs[i]``, as in ``compose(t, t, k)``): the reference's ``exp`` (src/tensors/ops_elementwise.cpp:174-223) -- combine
    codomain and domain into one pipe each, exponentiate every diagonal block, split again.  ALL blocks go through ONE
    ``bb.matrix_exp_many`` call (one launch if every block fits the in-LDS kernel); sectors without a block become
    identities.  A ``complex`` factor on a real tensor gives a complex result without a promotion pass.  Labels and
    ``num_codomain`` are kept.  A backend without ``matrix_exp_many`` runs ``bb.matrix_exp`` per block."""
    k = _square_half(t, 'exp')
    many = getattr(bb, 'matrix_exp_many', None)
    if many is not None:
        def method(entries):
            return many(entries, factor)
    else:
        def method(entries):
            blocks = [bb.zeros((e[0], e[0])) if isinstance(e, tuple) else e for e in entries]
            return [bb.matrix_exp(b) for b in bb.mul_many(factor, blocks)]
    return _on_square_matrix(bb, t, k, method)


def eye(bb, symmetry: Symmetry, legs, dtype=None) -> AbelianTensor:
    """The identity from `legs` to themselves (``eye_data``, include/cyten/backends/abelian.h:200): legs
    ``legs + [l.dual() for l in reversed(legs)]``, ``num_codomain = len(legs)``.  One ``eye_matrix`` block per sector of the
    pipe of `legs`, split into views."""
    legs = list(legs)
    if not legs:
        raise ValueError('eye: at least one leg')
    k = len(legs)
    lead = legs[0] if k == 1 else LegPipe.from_legs(symmetry, legs, +1)
    blocks = [bb.eye_matrix(int(m), dtype) for m in lead.mults]
    t = AbelianTensor(symmetry, [lead, lead.dual()], blocks, np.array([[j, j] for j in range(lead.nsec)], dtype=np.int64).reshape(lead.nsec, 2), 1)
    if k > 1:
        t = permute_legs(bb, split_legs(bb, t), list(range(k)) + list(range(2 * k - 1, k - 1, -1)), num_codomain=k)
    return t


_F0_NONZERO = ('exp', 'log', 'reciprocal')


def hermitian_function(bb, t: AbelianTensor, func: str, param=None) -> AbelianTensor:
    """``f(t)`` for a Hermitian tensor (leg requirements of :func:`exp`) through the eigendecomposition of its diagonal blocks,
    ``V f(w) V^dagger``: `func` is a name :func:`diagonal_unary` knows (exp, sqrt, log, stable_log, cutoff_inverse, pow, ...),
    applied to the real eigenvalues.  A fixed number of launches per tensor: ``eigh_batched``, ``unary_many`` on the list of
    eigenvalue vectors, ``scale_axis_many`` on the eigenvector columns, (complex blocks: one conjugating ``copy_many``) and ONE
    grouped GEMM with the adjoint views.  Functions with f(0) != 0 (exp, log, reciprocal, pow with an exponent <= 0) treat
    the sectors without a block as zero blocks, like :func:`act_block_diagonal_square_matrix`; the others leave them out.
    Hermiticity is the caller's promise: only what ``eigh`` reads of a block enters."""
    if func not in _UNARY_NAMES + _UNARY_PARAM_NAMES:
        raise ValueError(f'hermitian_function: unknown function {func!r}')
    k = _square_half(t, 'hermitian_function')
    all_sectors = func in _F0_NONZERO or (func == 'pow' and param is not None and param <= 0)

    def method(entries):
        missing = [i for i, e in enumerate(entries) if isinstance(e, tuple)]
        if missing:
            entries = list(entries)
            for i, z in zip(missing, bb.zeros_many([(entries[i][0],) * 2 for i in missing])):
                entries[i] = z
        wv = bb.eigh_batched(entries)
        fw = bb.unary_many([w for w, _ in wv], func, param)
        scaled = bb.scale_axis_many([(v, f, 1) for (_, v), f in zip(wv, fw)])
        adj = [bb.permute_axes(v, [1, 0]) for _, v in wv]
        todo = [i for i, a in enumerate(adj) if _is_complex_block(a)]
        if todo:
            new = bb.empty_many([adj[i].shape for i in todo], dtype='complex128')
            bb.copy_many([(d, adj[i]) for d, i in zip(new, todo)], conj=True)
            for d, i in zip(new, todo):
                adj[i] = d
        return bb.matrix_dot_grouped([[(x, a)] for x, a in zip(scaled, adj)])
    return _on_square_matrix(bb, t, k, method, all_sectors)


# ---------------------------------------------------------------------------------------------
# building operators: outer, direct_sum, tensor_from_grid, trivial legs
# ---------------------------------------------------------------------------------------------

def _relabelled(labels, mapping, n):
    labels = list(labels) if len(labels) == n else [None] * n
    return [mapping.get(l, l) for l in labels] if mapping else labels


def outer(bb, a: AbelianTensor, b: AbelianTensor, relabel_a=None, relabel_b=None) -> AbelianTensor:
    """The tensor product ``a (x) b`` (``AbelianBackend::outer``, abelian.cpp:2794-2850): legs ``a.legs[:K] + b.legs +
    a.legs[K:]`` with ``K = a.num_codomain``, ``num_codomain = K + b.num_codomain``; the block table is the F-style grid of
    all (a-block, b-block) pairs, lexsorted (the reference leaves it unsorted).  ALL blocks come from ONE
    ``bb.tensor_outer_many`` call, C-contiguous in their final axis order; a backend without that method runs
    ``tensor_outer`` + ``contiguous`` per pair.  `relabel_a` / `relabel_b` map old to new labels; a label that then occurs
    twice is a ``ValueError``.  Real next to complex gives a complex result."""
    if a.symmetry != b.symmetry:
        raise ValueError('outer: the tensors have different symmetries')
    na, nb, K = a.nlegs, b.nlegs, a.num_codomain
    if na + nb > CYB_MAX_NDIM:
        raise ValueError(f'outer: tensors of more than {CYB_MAX_NDIM} legs are not supported')
    labels = []
    if len(a.labels) == na or len(b.labels) == nb:
        la, lb = _relabelled(a.labels, relabel_a, na), _relabelled(b.labels, relabel_b, nb)
        labels = la[:K] + lb + la[K:]
        named = [l for l in labels if l is not None]
        if len(set(named)) != len(named):
            raise ValueError(f'outer: duplicate labels in {labels}')
    legs = list(a.legs[:K]) + list(b.legs) + list(a.legs[K:])
    l_a, l_b = len(a.blocks), len(b.blocks)
    ia, ib = np.tile(np.arange(l_a), l_b), np.repeat(np.arange(l_b), l_a)      # (first index fastest: make_grid(cstyle=False))
    rows = np.concatenate([a.block_inds[ia, :K], b.block_inds[ib], a.block_inds[ia, K:]], axis=1).reshape(l_a * l_b, na + nb)
    order = _lexsort_rows(rows)
    ia, ib, rows = ia[order], ib[order], rows[order]
    pairs = [(a.blocks[i], b.blocks[j]) for i, j in zip(ia.tolist(), ib.tolist())]
    many = getattr(bb, 'tensor_outer_many', None)
    if many is not None:
        blocks = many(pairs, K)
    else:
        cplx = any(_is_complex_block(x) for x in list(a.blocks) + list(b.blocks))
        blocks = [bb.contiguous(bb.tensor_outer(bb.as_complex(x) if cplx else x, bb.as_complex(y) if cplx else y, K)) for x, y in pairs]
    return AbelianTensor(a.symmetry, legs, list(blocks), rows, K + b.num_codomain, labels)


def direct_sum(legs) -> Leg:
    """``ElementarySpace.direct_sum``: the leg whose sectors are the union of the sectors of `legs` (same symmetry and sign),
    multiplicities added.  Pipes are refused: a sum of products is no product (constructors.cpp:364-367)."""
    legs = list(legs)
    if not legs:
        raise ValueError('direct_sum: at least one leg')
    first = legs[0]
    mults: dict = {}
    for l in legs:
        if isinstance(l, LegPipe):
            raise RuntimeError('stacking legs must be ElementarySpace')
        if l.symmetry != first.symmetry or l.sign != first.sign:
            raise ValueError('direct_sum: the legs must have the same symmetry and sign')
        for s, m in zip(l.sectors.tolist(), l.mults.tolist()):
            mults[tuple(s)] = mults.get(tuple(s), 0) + int(m)
    keys = list(mults)
    return Leg(first.symmetry, np.array(keys, dtype=np.int64).reshape(len(keys), first.symmetry.n), [mults[k] for k in keys], first.sign)


_GRID_CACHE: dict = {}


def _sector_where(leg: Leg) -> dict:
    return {tuple(s): i for i, s in enumerate(leg.sectors.tolist())}


def _mult_slices(total: Leg, spaces):
    """per sector of `total` the cumulative sums (leading zero) of its multiplicity in each of `spaces` (constructors.cpp:439-460)"""
    wheres = [_sector_where(s) for s in spaces]
    out = []
    for sec in total.sectors.tolist():
        m = [int(sp.mults[w[tuple(sec)]]) if tuple(sec) in w else 0 for sp, w in zip(spaces, wheres)]
        out.append([0] + np.cumsum(m).tolist())
    return out


def tensor_from_grid(bb, grid, labels=None, dtype=None) -> AbelianTensor:
    """Stack a grid of tensors into one (``tensor_from_grid``, src/tensors/constructors.cpp:304-499, on
    ``AbelianBackend::from_grid``, abelian.cpp:1875-1978): `grid` is a list of rows of ``AbelianTensor | None``; the rows stack
    on leg 0, the columns on leg ``num_codomain``, every other leg is equal across the entries.  The stacked legs are the
    :func:`direct_sum` of one representative per row / column (the entry of the first column / row, else the first entry
    found), and an entry occupies, in every sector, the slice its row / column has in the cumulative multiplicities.

    Cells never overlap, so every block is *copied* to its place (the reference adds into zeros): one ``zeros_many``
    (``empty_many`` if the cells cover the result) and ONE placement launch for the whole grid from a device-resident
    plan cached by structure, as :func:`combine_legs` does; views are read through their strides.  A backend without plans
    takes ``zeros_many`` + one ``copy_many``.  Real next to complex entries (or ``dtype='complex128'``) give complex128."""
    grid = [list(row) for row in grid]
    ops = [op for row in grid for op in row if op is not None]
    if not ops:
        raise ValueError('grid must contain at least one tensor')
    ref = ops[0]
    sym, n, n_cod = ref.symmetry, ref.nlegs, ref.num_codomain
    if n_cod < 1 or n - n_cod < 1:
        raise ValueError('tensor_from_grid: the entries need at least one codomain and one domain leg')
    if n > CYB_MAX_NDIM:
        raise ValueError(f'tensor_from_grid: tensors of more than {CYB_MAX_NDIM} legs are not supported')
    others = [k for k in range(n) if k not in (0, n_cod)]
    for op in ops:
        if op.symmetry != sym:
            raise ValueError('tensor_from_grid: the entries have different symmetries')
        if op.nlegs != n or op.num_codomain != n_cod:
            raise RuntimeError('inconsistent number of legs in grid')
        if not all(_same_leg(op.legs[k], ref.legs[k]) for k in others):
            raise RuntimeError('inconsistent legs in grid')
        if isinstance(op.legs[0], LegPipe) or isinstance(op.legs[n_cod], LegPipe):
            raise RuntimeError('stacking legs must be ElementarySpace')
    n_rows, n_cols = len(grid), len(grid[0])
    if any(len(row) != n_cols for row in grid):
        raise ValueError('grid rows must have equal length')
    right_ops = [next((grid[r][j] for r in range(n_rows) if grid[r][j] is not None), None) for j in range(n_cols)]
    if any(op is None for op in right_ops):
        raise ValueError('Must have at least one nonzero entry in each column.')
    left_ops = [next((op for op in row if op is not None), None) for row in grid]
    if any(op is None for op in left_ops):
        raise ValueError('Must have at least one nonzero entry in each row.')
    left_spaces, right_spaces = [op.legs[0] for op in left_ops], [op.legs[n_cod] for op in right_ops]
    cells = [(i, j, op) for i, row in enumerate(grid) for j, op in enumerate(row) if op is not None]
    for i, j, op in cells:        # (the reference trusts this; a cell of another size would be placed outside its slice)
        if not _same_leg(op.legs[0], left_spaces[i]) or not _same_leg(op.legs[n_cod], right_spaces[j]):
            raise RuntimeError('inconsistent legs in grid')
    left, right = direct_sum(left_spaces), direct_sum(right_spaces)
    legs = [left] + list(ref.legs[1:n_cod]) + [right] + list(ref.legs[n_cod + 1:])
    if labels is None:
        labels = list(ref.labels) if len(ref.labels) == n else []
    elif len(labels) != n:
        raise ValueError(f'tensor_from_grid: {n} labels expected')
    blocks = [b for _, _, op in cells for b in op.blocks]
    want_cplx = dtype is not None and np.dtype(dtype).kind == 'c'
    if dtype is not None and not want_cplx and any(_is_complex_block(b) for b in blocks):
        raise ValueError('tensor_from_grid: complex entries cannot be stored in a real dtype')
    if not blocks:
        return AbelianTensor(sym, legs, [], np.zeros((0, n), np.int64), n_cod, list(labels))
    blocks, cplx = _promote_mixed(bb, blocks)
    if want_cplx and not cplx:
        blocks, cplx = [bb.as_complex(b) for b in blocks] if not hasattr(bb, 'as_complex_many') else bb.as_complex_many(blocks), True
    esz = 16 if cplx else 8
    native = _has_plans(bb)
    key = (n_cod, n_rows, n_cols, esz, _block_strides(bb, blocks),
           tuple((i, j, _legs_key(sym, op.legs, [l.sign for l in op.legs]), np.ascontiguousarray(op.block_inds).tobytes()) for i, j, op in cells))
    plan = _GRID_CACHE.get(key)
    if plan is None:
        plan = _cache_put(_GRID_CACHE, key, _grid_plan(cells, legs, n_cod, _mult_slices(left, left_spaces), _mult_slices(right, right_spaces),
                                                       [tuple(b.strides) for b in blocks] if native else None))
    new_rows, new_shapes = plan['rows'], plan['shapes']
    dt = 'complex128' if cplx else None
    if native:
        if plan.get('native') is None:
            plan['native'] = bb.place_plan(plan['records'], len(blocks), len(new_shapes), esz)
        new_blocks = bb.empty_many(new_shapes, dtype=dt) if plan['covers'] else bb.zeros_many(new_shapes, dtype=dt)
        bb.place_enqueue(plan['native'], [b.ptr for b in blocks], [b.ptr for b in new_blocks])
    else:
        new_blocks = bb.zeros_many(new_shapes, dtype=dt)
        bb.copy_many([(bb.get_item(new_blocks[dst], key_sl), blk) for blk, (dst, key_sl) in zip(blocks, plan['generic'])])
    return AbelianTensor(sym, legs, list(new_blocks), new_rows.copy(), n_cod, list(labels))


def _grid_plan(cells, legs, n_cod, left_slices, right_slices, src_strides):
    """The placement of one grid structure: result block table (lexsorted, no duplicates), result shapes and per entry block
    its result block and slice -- as placement records (`src_strides` given) and as slices for the generic route."""
    n = len(legs)
    left_where, right_where = _sector_where(legs[0]), _sector_where(legs[n_cod])
    rows, spans, ext = [], [], []
    for i, j, op in cells:
        l0, lc = op.legs[0], op.legs[n_cod]
        for row in op.block_inds.tolist():
            li, ri = left_where[tuple(l0.sectors[row[0]].tolist())], right_where[tuple(lc.sectors[row[n_cod]].tolist())]
            rows.append([li] + row[1:n_cod] + [ri] + row[n_cod + 1:])
            spans.append((left_slices[li][i], left_slices[li][i + 1], right_slices[ri][j], right_slices[ri][j + 1]))
            ext.append([int(l.mults[k]) for l, k in zip(op.legs, row)])
    rows = np.array(rows, dtype=np.int64).reshape(len(rows), n)
    order = _lexsort_rows(rows)
    srt = rows[order]
    is_new = np.concatenate([[True], np.any(srt[1:] != srt[:-1], axis=1)])
    new_of = np.zeros(len(rows), dtype=np.int64)
    new_of[order] = np.cumsum(is_new) - 1
    new_rows = srt[is_new]
    shapes = [tuple(int(l.mults[k]) for l, k in zip(legs, row)) for row in new_rows.tolist()]
    out = dict(rows=new_rows, shapes=shapes, generic=[], records=None, native=None)
    recs = _place_records(len(rows)) if src_strides is not None else None
    placed = 0
    for b in range(len(rows)):
        dst = int(new_of[b])
        r0, r1, c0, c1 = spans[b]
        placed += math.prod(ext[b])
        out['generic'].append((dst, tuple(slice(r0, r1) if k == 0 else (slice(c0, c1) if k == n_cod else slice(None)) for k in range(n))))
        if recs is not None:
            dstr = _c_strides_of(shapes[dst])
            rec = recs[b]
            rec['src_block'], rec['dst_block'], rec['ndim'], rec['dst_offset'] = b, dst, n, r0 * dstr[0] + c0 * dstr[n_cod]
            rec['shape'][:n], rec['src_strides'][:n], rec['dst_strides'][:n] = ext[b], src_strides[b], dstr
    out['records'] = recs
    out['covers'] = placed == sum(math.prod(sh) for sh in shapes)    # (cells never overlap: equal sizes = all covered)
    return out


def add_trivial_leg(bb, t: AbelianTensor, pos: int, to_domain: bool = False, label=None) -> AbelianTensor:
    """A leg with the one sector of charge 0, multiplicity 1, inserted at position `pos` of the flat leg list
    (``AbelianBackend::add_trivial_leg``, abelian.cpp:596-613): metadata only -- ``bb.add_axis`` per block and a constant column
    in the block table, which stays sorted.  In the codomain (``pos <= num_codomain``, not `to_domain`) the leg has sign +1
    and ``num_codomain`` grows; in the domain (``pos >= num_codomain``) it has sign -1."""
    n, K = t.nlegs, t.num_codomain
    pos = int(pos)
    if not 0 <= pos <= n:
        raise ValueError(f'add_trivial_leg: position {pos} outside [0, {n}]')
    if (to_domain and pos < K) or (not to_domain and pos > K):
        raise ValueError(f'add_trivial_leg: position {pos} does not lie in the {"domain" if to_domain else "codomain"}')
    leg = Leg(t.symmetry, np.zeros((1, t.symmetry.n), dtype=np.int64), [1], -1 if to_domain else +1)
    labels = list(t.labels[:pos]) + [label] + list(t.labels[pos:]) if len(t.labels) == n else ([] if label is None else [None] * pos + [label] + [None] * (n - pos))
    return AbelianTensor(t.symmetry, list(t.legs[:pos]) + [leg] + list(t.legs[pos:]), [bb.add_axis(b, pos) for b in t.blocks],
                         np.insert(t.block_inds, pos, 0, axis=1), K + (0 if to_domain else 1), labels)


def _is_trivial_leg(symmetry: Symmetry, leg: Leg) -> bool:
    return leg.nsec == 1 and int(leg.mults[0]) == 1 and not np.any(leg.sectors)


def squeeze_legs(bb, t: AbelianTensor, idcs=None) -> AbelianTensor:
    """Remove trivial legs (one sector of charge 0, multiplicity 1), by default all of them (``AbelianBackend::squeeze_legs``,
    abelian.cpp:3439-3458): metadata only -- ``bb.squeeze_axes`` per block, the columns deleted from the block table.  A listed
    leg that is not trivial is a ``ValueError``."""
    n = t.nlegs
    if idcs is None:
        idcs = [k for k in range(n) if _is_trivial_leg(t.symmetry, t.legs[k])]
    elif isinstance(idcs, (int, np.integer)):
        idcs = [int(idcs)]
    idcs = sorted({int(i) % n for i in idcs})
    for k in idcs:
        if not _is_trivial_leg(t.symmetry, t.legs[k]):
            raise ValueError(f'squeeze_legs: leg {k} is not trivial')
    keep = [k for k in range(n) if k not in idcs]
    blocks = [bb.squeeze_axes(b, idcs) for b in t.blocks] if idcs else list(t.blocks)
    return AbelianTensor(t.symmetry, [t.legs[k] for k in keep], blocks, t.block_inds[:, keep].reshape(len(blocks), len(keep)),
                         t.num_codomain - sum(1 for k in idcs if k < t.num_codomain), [t.labels[k] for k in keep] if len(t.labels) == n else [])


# ---------------------------------------------------------------------------------------------
# diagonal-tensor arithmetic, reductions and device-side masks
# ---------------------------------------------------------------------------------------------

_ARITH_OPS = ('add', 'sub', 'mul', 'div')
_COMPARE_OPS = ('lt', 'le', 'gt', 'ge', 'eq', 'ne')
_LOGICAL_OPS = ('and', 'or', 'xor')
_PY_COMPARE = {'lt': lambda a, b: a < b, 'le': lambda a, b: a <= b, 'gt': lambda a, b: a > b, 'ge': lambda a, b: a >= b,
               'eq': lambda a, b: a == b, 'ne': lambda a, b: a != b}


def _by_sector(blocks, inds) -> dict:
    return {int(i): b for i, b in zip(inds, blocks)}


def _parse_index(leg: Leg, idx: int):
    """(sector index, index within the sector) of basis state `idx` of `leg` (``Space.parse_index``)"""
    idx = int(idx)
    if idx < 0:
        idx += leg.dim
    if not 0 <= idx < leg.dim:
        raise IndexError(f'index {idx} out of range for a leg of dimension {leg.dim}')
    sec = int(np.searchsorted(np.asarray(leg.slices), idx, side='right')) - 1
    return sec, idx - int(leg.slices[sec])


def _binary_result_dtype(func: str, dtype_a, dtype_b) -> np.dtype:
    """dtype of ``func(ones(dtype_a), ones(dtype_b))``: the reference's sample rule for a result without blocks
    (abelian.cpp:1622-1626)"""
    if func in _ARITH_OPS:
        return np.dtype(np.complex128 if 'c' in (np.dtype(dtype_a).kind, np.dtype(dtype_b).kind) else np.float64)
    return np.dtype(np.bool_)


def diagonal_binary(bb, a: DiagonalTensor, b: DiagonalTensor, func: str, partial_zero_is_zero: bool) -> DiagonalTensor:
    """``AbelianBackend::diagonal_elementwise_binary`` (abelian.cpp:1568-1633) for the functions the device serves by name:
    add, sub, mul, div; lt, le, gt, ge, eq, ne; and, or, xor (boolean diagonals).  The merge over the sectors of the leg is
    the reference's (:1596-1619): with `partial_zero_is_zero` a sector missing on either side is skipped; otherwise the
    missing operand is the kernel's "absent" kind, read as zeros -- no zero block is allocated (:1605, :1615).  ALL sectors
    are ONE ``seg_binary_many`` launch and no download, where the reference calls ``func`` per sector.  A result without
    blocks gets its dtype from the sample rule (:1622-1626).  (Where `a` lacks a sector that `b` has, the reference skips the
    sector without stepping over the block of `b` (:1602-1603) and then treats every later block of `b` as missing; the
    stated rule is followed here, not that slip.)"""
    if func not in _ARITH_OPS + _COMPARE_OPS + _LOGICAL_OPS:
        raise ValueError(f'diagonal_binary: unknown function {func!r}')
    if a.symmetry != b.symmetry or not _same_space(a.leg, b.leg):
        raise ValueError('diagonal_binary: the two diagonals do not live on the same leg')
    ha, hb = _by_sector(a.blocks, a.block_inds), _by_sector(b.blocks, b.block_inds)
    items, inds = [], []
    for i in range(a.leg.nsec):
        blk_a, blk_b = ha.get(i), hb.get(i)
        if partial_zero_is_zero and (blk_a is None or blk_b is None):
            continue
        items.append((blk_a, blk_b, int(a.leg.mults[i])))
        inds.append(i)
    dtype = _binary_result_dtype(func, a.dtype, b.dtype)
    blocks = bb.seg_binary_many(items, func, complex_out=dtype.kind == 'c') if items else []
    return DiagonalTensor(a.symmetry, a.leg, list(blocks), np.array(inds, dtype=np.int64), dtype)


def diagonal_compare(bb, d: DiagonalTensor, op: str, scalar) -> DiagonalTensor:
    """``d (op) scalar`` as a boolean DiagonalTensor (``DiagonalTensor._elementwise_binary`` with a number, through
    abelian.cpp:743-782 with ``maps_zero_to_zero`` decided by ``0 (op) scalar``): a sector without a block compares as
    zeros, so it gets an all-true block if ``0 (op) scalar`` holds and stays without a block (all false) otherwise -- the
    absent kind again, no zero block.  ONE launch for all sectors, no download."""
    if op not in _COMPARE_OPS:
        raise ValueError(f'diagonal_compare: unknown comparison {op!r}')
    if isinstance(scalar, complex) and op not in ('eq', 'ne'):
        raise TypeError('diagonal_compare: complex numbers are not ordered')
    have = _by_sector(d.blocks, d.block_inds)
    fill = bool(_PY_COMPARE[op](0.0, scalar))
    items, inds = [], []
    for i in range(d.leg.nsec):
        if i in have or fill:
            items.append((have.get(i), None, int(d.leg.mults[i])))
            inds.append(i)
    blocks = bb.seg_binary_many(items, op, scalar=scalar) if items else []
    return DiagonalTensor(d.symmetry, d.leg, list(blocks), np.array(inds, dtype=np.int64), np.bool_)


def _counts(bb, d: DiagonalTensor) -> np.ndarray:
    table = bb.seg_reduce_many(d.blocks, [int(d.leg.mults[i]) for i in d.block_inds], 'count')
    return table[:, 0].astype(np.int64)


def diagonal_all(bb, d: DiagonalTensor) -> bool:
    """``AbelianBackend::diagonal_all`` (abelian.cpp:717-730): missing blocks are False (:724), the existing ones must be
    all-true -- ONE counting launch and one download instead of ``all(block)`` per sector (:726-728)."""
    if len(d.blocks) < d.leg.nsec:
        return False
    if not d.blocks:
        return True
    return bool(np.all(_counts(bb, d) == np.asarray(d.leg.mults)[d.block_inds]))


def diagonal_any(bb, d: DiagonalTensor) -> bool:
    """``AbelianBackend::diagonal_any`` (abelian.cpp:733-740): ONE counting launch instead of ``any(block)`` per sector."""
    return bool(d.blocks) and bool(np.any(_counts(bb, d) > 0))


_REDUCERS = {'sum': lambda xs: sum(xs[1:], xs[0]) if len(xs) else 0.0, 'max': max, 'min': min}


def _numbers(table: np.ndarray, cplx: bool) -> list:
    return [complex(re, im) for re, im in table] if cplx else [float(re) for re in table[:, 0]]


def reduce_diagonal(bb, d: DiagonalTensor, block_func: str, func=None):
    """``AbelianBackend::reduce_DiagonalTensor`` (abelian.cpp:3154-3175): `block_func` (sum, max, min) of EVERY sector of
    the leg -- a sector without a block is reduced as zeros of its multiplicity (:3170), the absent kind -- by ONE
    ``seg_reduce_many`` launch and one download of ``16 * n_sectors`` bytes, then ``func(numbers)`` on the host in ascending
    sector order (:3174).  `func`: a callable on the list of numbers, or None for the reduction named by `block_func`."""
    if block_func not in _REDUCERS:
        raise ValueError(f'reduce_diagonal: unknown block function {block_func!r}')
    if block_func != 'sum' and d.dtype.kind == 'c':
        raise TypeError('reduce_diagonal: complex numbers are not ordered')
    have = _by_sector(d.blocks, d.block_inds)
    table = bb.seg_reduce_many([have.get(i) for i in range(d.leg.nsec)], [int(m) for m in d.leg.mults], block_func)
    numbers = _numbers(table, d.dtype.kind == 'c')
    return (_REDUCERS[block_func] if func is None else func)(numbers)


def diagonal_trace_full(bb, d: DiagonalTensor):
    """``AbelianBackend::diagonal_tensor_trace_full`` (abelian.cpp:966-973): the sum of ``sum_all`` over the blocks, in
    block order, from ONE launch and one download instead of a launch and a synchronisation per block (:970-971)."""
    total = 0j if d.dtype.kind == 'c' else 0.0
    if d.blocks:
        table = bb.seg_reduce_many(d.blocks, [int(d.leg.mults[i]) for i in d.block_inds], 'sum')
        for x in _numbers(table, d.dtype.kind == 'c'):
            total = total + x
    return total


def get_element_diagonal(bb, d: DiagonalTensor, idx: int):
    """``AbelianBackend::get_element_diagonal`` (abelian.cpp:2118-2131); zero of the dtype if the sector has no block"""
    sec, within = _parse_index(d.leg, idx)
    blk = _by_sector(d.blocks, d.block_inds).get(sec)
    if blk is None:
        return d.dtype.type(0).item()
    return np.asarray(bb.to_numpy(bb.get_item(blk, (slice(within, within + 1),)))).reshape(()).item()


def _leg_slice(leg: Leg, i) -> slice:
    return slice(int(leg.slices[int(i)]), int(leg.slices[int(i) + 1]))


def diagonal_to_block(bb, d: DiagonalTensor):
    """``AbelianBackend::diagonal_tensor_to_block`` (abelian.cpp:1679-1692): the full diagonal as ONE 1-D block -- one
    memset plus one batched copy instead of ``res[slice] = block`` per sector (:1686-1690)."""
    res = bb.zeros_many([(d.leg.dim,)], dtype=d.dtype)[0]
    pairs = [(bb.get_item(res, (_leg_slice(d.leg, i),)), blk) for blk, i in zip(d.blocks, d.block_inds)]
    if pairs:
        bb.copy_many(pairs)
    return res


def _diagonal_block_inds(t: AbelianTensor, what: str) -> np.ndarray:
    if t.nlegs != 2 or not _same_space(t.legs[0], t.legs[1]):
        raise ValueError(f'{what}: a tensor with two legs over the same sectors and multiplicities is required')
    if len(t.blocks) and not np.array_equal(t.block_inds[:, 0], t.block_inds[:, 1]):
        raise ValueError(f'{what}: the tensor has blocks off the diagonal of its block table')
    return t.block_inds[:, 0].copy() if len(t.blocks) else np.zeros(0, np.int64)


def diagonal_from_full_tensor(bb, t: AbelianTensor, tol=None) -> DiagonalTensor:
    """``AbelianBackend::diagonal_tensor_from_full_tensor`` (abelian.cpp:956-963): the diagonals of ALL blocks by ONE batched
    strided copy (source stride ``s0 + s1``) where the reference calls ``get_diagonal`` per block (:960-961).  With `tol`
    the off-diagonal entries of all blocks -- for a contiguous ``n x n`` block they are ONE ``(n - 1, n)`` view with strides
    ``(n + 1, 1)`` -- go through one further grouped reduction and one download; ``ValueError('Not a diagonal block.')`` if
    one of them exceeds `tol`, as ``get_diagonal`` raises per block."""
    inds = _diagonal_block_inds(t, 'diagonal_from_full_tensor')
    if tol is not None and t.blocks:
        offs = [bb.off_diagonal_view(b) for b in bb.contiguous_many(list(t.blocks))]
        if not bb.max_abs_many([o for o in offs if o.size]) <= tol:
            raise ValueError('Not a diagonal block.')
    cplx = any(_is_complex_block(b) for b in t.blocks)
    outs = bb.empty_many([(int(t.legs[0].mults[i]),) for i in inds], dtype='complex128' if cplx else None) if len(inds) else []
    if len(inds):
        bb.copy_many([(o, bb.diagonal_view(b if not cplx or _is_complex_block(b) else bb.as_complex(b))) for o, b in zip(outs, t.blocks)])
    return DiagonalTensor(t.symmetry, t.legs[0], list(outs), inds)


def full_from_diagonal(bb, d: DiagonalTensor) -> AbelianTensor:
    """``AbelianBackend::full_data_from_diagonal_tensor`` (abelian.cpp:936-943) as the tensor ``[leg, leg*]``: one zero fill
    plus one batched strided copy onto the diagonals instead of ``block_from_diagonal`` per block (:940-941)."""
    if d.dtype.kind == 'b':
        raise TypeError('full_from_diagonal: convert a boolean diagonal with mask_to_diagonal / diagonal_binary first')
    blocks = bb.zeros_many([(int(d.leg.mults[i]),) * 2 for i in d.block_inds], dtype='complex128' if d.dtype.kind == 'c' else None) if d.blocks else []
    if d.blocks:
        bb.copy_many([(bb.diagonal_view(o), b) for o, b in zip(blocks, d.blocks)])
    inds = np.stack([d.block_inds, d.block_inds], axis=1).reshape(len(d.blocks), 2)
    return AbelianTensor(d.symmetry, [d.leg, d.leg.dual()], list(blocks), inds, 1)


def diagonal_transpose(bb, d: DiagonalTensor) -> DiagonalTensor:
    """``AbelianBackend::diagonal_transpose`` (abelian.cpp:1009-1016): the same blocks on the dual leg -- metadata only
    (blocks are values here, the reference's copy is not needed)."""
    return DiagonalTensor(d.symmetry, d.leg.dual(), list(d.blocks), d.block_inds.copy(), d.dtype)


# -- masks

def _device_mask(large_leg: Leg, flag_blocks, large_inds, tables, counts, is_projection=True) -> Mask:
    """the Mask of the sectors of `large_inds` that keep at least one state (abelian.cpp:1730-1755 / :2441-2468; there is no
    basis permutation in this project)"""
    keep = [k for k in range(len(flag_blocks)) if int(counts[k]) > 0]
    sectors = large_leg.sectors[[int(large_inds[k]) for k in keep]].reshape(len(keep), large_leg.symmetry.n)
    small = Leg(large_leg.symmetry, sectors, [int(counts[k]) for k in keep], large_leg.sign)
    inds = np.array([[j, int(large_inds[k])] for j, k in enumerate(keep)], dtype=np.int64).reshape(len(keep), 2)
    if not is_projection:
        inds = inds[:, ::-1].copy()
    return Mask(large_leg, small, [flag_blocks[k] for k in keep], inds, [tables[k] for k in keep], is_projection)


def diagonal_to_mask(bb, d: DiagonalTensor) -> Mask:
    """``AbelianBackend::diagonal_to_mask`` (abelian.cpp:1695-1756) for a boolean diagonal: ONE ``seg_compact_many`` over the
    blocks of `d` writes the position table of every sector on the device; the host reads the kept counts (one download of
    ``8 * n_blocks`` bytes), drops the all-false sectors and builds the small leg (:1707-1755).  The reference calls
    ``any``, ``sum_all`` and ``to_numpy`` per sector (:1709-1728).  The flag blocks and the tables stay on the device."""
    if d.dtype.kind != 'b':
        raise TypeError('diagonal_to_mask: a boolean DiagonalTensor is required')
    tables, counts = bb.seg_compact_many(list(d.blocks)) if d.blocks else ([], np.zeros(0, np.int64))
    return _device_mask(d.leg, list(d.blocks), d.block_inds, tables, counts)


def _mask_logic(bb, items, large_leg: Leg, func: str) -> Mask:
    flags = bb.seg_binary_many(items, func) if items else []
    tables, counts = bb.seg_compact_many(list(flags)) if flags else ([], np.zeros(0, np.int64))
    return _device_mask(large_leg, list(flags), np.arange(large_leg.nsec), tables, counts)


def mask_binary(bb, m1: Mask, m2: Mask, func: str) -> Mask:
    """``AbelianBackend::mask_binary_operand`` (abelian.cpp:2385-2469), `func` one of and, or, xor: ONE ``seg_binary_many``
    over ALL sectors of the large leg (a sector without a block is the absent kind, where the reference allocates zero blocks,
    :2417, :2425), then ONE ``seg_compact_many`` whose counts -- the only download -- decide which sectors keep a block and
    give the multiplicities of the small leg (the reference: ``sum_all`` per sector, :2428)."""
    if func not in _LOGICAL_OPS:
        raise ValueError(f'mask_binary: unknown function {func!r}')
    if not (m1.is_projection and m2.is_projection):
        raise ValueError('mask_binary: projections are required')
    if m1.large_leg.symmetry != m2.large_leg.symmetry or not _same_space(m1.large_leg, m2.large_leg):
        raise ValueError('mask_binary: the masks do not have the same large leg')
    h1, h2 = _by_sector(m1.blocks, m1.block_inds[:, 1]), _by_sector(m2.blocks, m2.block_inds[:, 1])
    leg = m1.large_leg
    return _mask_logic(bb, [(_flag_block(bb, h1.get(i)), _flag_block(bb, h2.get(i)), int(leg.mults[i])) for i in range(leg.nsec)], leg, func)


def mask_unary(bb, m: Mask, func: str = 'not') -> Mask:
    """``AbelianBackend::mask_unary_operand`` (abelian.cpp:2686-2757) for ``logical_not``: as :func:`mask_binary`, two launches
    and one download.  The sectors that have a block change: a sector the mask keeps whole loses its block, a sector the
    mask drops whole (no block) gets an all-true one."""
    if func != 'not':
        raise ValueError(f'mask_unary: unknown function {func!r}')
    if not m.is_projection:
        raise ValueError('mask_unary: a projection is required')
    have = _by_sector(m.blocks, m.block_inds[:, 1])
    leg = m.large_leg
    return _mask_logic(bb, [(_flag_block(bb, have.get(i)), None, int(leg.mults[i])) for i in range(leg.nsec)], leg, func)


def _flag_block(bb, b):
    """a mask block as the backend's boolean block (the blocks of ``Mask.from_flags`` are host vectors)"""
    return b if b is None or bb.is_correct_block_type(b) else bb.as_block(np.asarray(b, dtype=bool))


def mask_dagger(bb, m: Mask) -> Mask:
    """``AbelianBackend::mask_dagger`` (abelian.cpp:976-985): the legs change places, i.e. the two columns of ``block_inds``
    (both ascending, so the table stays sorted) and the projection flag; blocks and tables are shared."""
    return Mask(m.large_leg, m.small_leg, list(m.blocks), m.block_inds[:, ::-1].copy(), m.tables, not m.is_projection)


def mask_transpose(bb, m: Mask) -> Mask:
    """``AbelianBackend::mask_transpose`` (abelian.cpp:2674-2683): as the dagger, on the dual legs"""
    return Mask(m.large_leg.dual(), m.small_leg.dual(), list(m.blocks), m.block_inds[:, ::-1].copy(), m.tables, not m.is_projection)


def get_element_mask(bb, m: Mask, idcs) -> bool:
    """``AbelianBackend::get_element_mask`` (abelian.cpp:2133-2156): `idcs` in the leg order of the mask, (small, large) for a
    projection and (large, small) for an inclusion"""
    legs = [m.small_leg, m.large_leg] if m.is_projection else [m.large_leg, m.small_leg]
    if len(idcs) != 2:
        raise ValueError('get_element_mask: two indices are required')
    pos = [_parse_index(l, i) for l, i in zip(legs, idcs)]
    hit = [j for j, row in enumerate(m.block_inds) if (int(row[0]), int(row[1])) == (pos[0][0], pos[1][0])]
    if not hit:
        return False
    small, large = (pos[0][1], pos[1][1]) if m.is_projection else (pos[1][1], pos[0][1])
    flags = np.asarray(bb.to_numpy(m.blocks[hit[0]]) if bb.is_correct_block_type(m.blocks[hit[0]]) else m.blocks[hit[0]]).astype(bool)
    return bool(flags[large]) and small == int(flags[:large].sum())


def mask_to_block(bb, m: Mask):
    """``AbelianBackend::mask_to_block`` (abelian.cpp:2641-2657): ONE boolean block over the large leg, one memset plus one
    batched copy"""
    res = bb.zeros_many([(m.large_leg.dim,)], dtype=bool)[0]
    pairs = [(bb.get_item(res, (_leg_slice(m.large_leg, row[m.large_col]),)), _flag_block(bb, blk)) for blk, row in zip(m.blocks, m.block_inds)]
    if pairs:
        bb.copy_many(pairs)
    return res


def mask_to_diagonal(bb, m: Mask, dtype=np.float64) -> DiagonalTensor:
    """``AbelianBackend::mask_to_diagonal`` (abelian.cpp:2659-2672): the flags as numbers on the large leg; the conversion of
    all blocks is ONE launch (the flags times 1.0) instead of ``to_dtype`` per block (:2665-2666)."""
    dtype = np.dtype(dtype)
    inds = m.block_inds[:, m.large_col].copy()
    blocks = [_flag_block(bb, b) for b in m.blocks]
    if dtype.kind != 'b' and blocks:
        blocks = bb.seg_binary_many([(b, None, int(m.large_leg.mults[i])) for b, i in zip(blocks, inds)], 'mul', scalar=1.0)
        if dtype.kind == 'c':
            blocks = [bb.as_complex(b) for b in blocks]
    return DiagonalTensor(m.large_leg.symmetry, m.large_leg, list(blocks), inds, dtype)


def full_from_mask(bb, m: Mask, dtype=np.float64) -> AbelianTensor:
    """``AbelianBackend::full_data_from_mask`` (abelian.cpp:945-953): the mask as the tensor ``[small, large*]`` (or its
    dagger), every block ``(k, n)`` with a single 1 per row at the kept positions.  Identity blocks (one zero fill, one
    batched copy of ones onto the diagonals) are scattered along their columns by ONE ``enlarge_leg_many`` that reads the
    position tables of a device mask in place; the reference calls ``block_from_mask`` per block (:950-951)."""
    ks = [int(m.small_leg.mults[int(row[1 - m.large_col])]) for row in m.block_inds]
    ns = [int(m.large_leg.mults[int(row[m.large_col])]) for row in m.block_inds]
    blocks = []
    if ks:
        eyes = bb.zeros_many([(k, k) for k in ks])
        ones = bb.seg_binary_many([(None, None, max(ks))], 'add', scalar=1.0)[0]
        bb.copy_many([(bb.diagonal_view(e), bb.get_item(ones, (slice(0, k),))) for e, k in zip(eyes, ks)])
        which = m.tables if m.tables is not None else [np.flatnonzero(np.asarray(b, dtype=bool)) for b in m.blocks]
        blocks = bb.enlarge_leg_many([(e, (w, n), 1) for e, w, n in zip(eyes, which, ns)])
        if not m.is_projection:
            blocks = [bb.permute_axes(b, [1, 0]) for b in blocks]
        if np.dtype(dtype).kind == 'c':
            blocks = [bb.as_complex(b) for b in blocks]
    legs = [m.small_leg, m.large_leg.dual()] if m.is_projection else [m.large_leg, m.small_leg.dual()]
    return AbelianTensor(m.large_leg.symmetry, legs, list(blocks), m.block_inds.copy().reshape(len(ks), 2), 1)


def apply_mask_to_diagonal(bb, d: DiagonalTensor, mask: Mask) -> DiagonalTensor:
    """``AbelianBackend::apply_mask_to_DiagonalTensor`` (abelian.cpp:646-673): the sectors `d` and the mask share (:658-669)
    go through ONE ``mask_gather_many`` instead of ``apply_mask`` per sector (:663-666); the result lives on the small leg."""
    items, inds = _apply_mask_items(d, mask)
    blocks = bb.mask_gather_many(items) if items else []
    return DiagonalTensor(d.symmetry, mask.small_leg, list(blocks), np.array(inds, dtype=np.int64), d.dtype)


def _apply_mask_items(d: DiagonalTensor, mask: Mask):
    if not mask.is_projection:
        raise ValueError('apply_mask_to_diagonal: a projection is required')
    if d.symmetry != mask.large_leg.symmetry or not _same_space(d.leg, mask.large_leg):
        raise ValueError('apply_mask_to_diagonal: the leg of the diagonal is not the large leg of the mask')
    have = _by_sector(d.blocks, d.block_inds)
    items, inds = [], []
    for j, row in enumerate(mask.block_inds):
        blk = have.get(int(row[1]))
        if blk is not None:
            items.append((blk, mask.tables[j] if mask.tables is not None else mask.blocks[j], 0))
            inds.append(int(row[0]))
    return items, inds


def svd_apply_mask(bb, U: AbelianTensor, S: DiagonalTensor, Vh: AbelianTensor, mask: Mask):
    """``svd_apply_mask`` (src/tensors/decompositions.cpp:620-631): project the new leg of ``U`` (its last leg), of ``S`` and
    of ``Vh`` (its first leg) onto the states the mask keeps.  The reference composes U with the dagger of the mask, applies
    the mask to S and composes it with Vh, each a loop over blocks; here the three block tables are matched on the host and
    the blocks of all three go through ONE ``mask_gather_many`` call, which reads the position tables of a device mask in
    place (no upload of index tables)."""
    if not mask.is_projection:
        raise ValueError('svd_apply_mask: a projection is required')
    u_items, u_rows, u_legs = _mask_contract_items(U, mask, U.nlegs - 1, True)
    s_items, s_inds = _apply_mask_items(S, mask)
    v_items, v_rows, v_legs = _mask_contract_items(Vh, mask, 0, True)
    items = u_items + s_items + v_items
    out = bb.mask_gather_many(items) if items else []
    nu, ns = len(u_items), len(s_items)
    U2 = AbelianTensor(U.symmetry, u_legs, list(out[:nu]), np.array(u_rows, dtype=np.int64).reshape(nu, U.nlegs), U.num_codomain, list(U.labels)).sorted()
    S2 = DiagonalTensor(S.symmetry, mask.small_leg, list(out[nu:nu + ns]), np.array(s_inds, dtype=np.int64), S.dtype)
    V2 = AbelianTensor(Vh.symmetry, v_legs, list(out[nu + ns:]), np.array(v_rows, dtype=np.int64).reshape(len(v_items), Vh.nlegs), Vh.num_codomain,
                       list(Vh.labels)).sorted()
    return U2, S2, V2


def entropy(bb, p: DiagonalTensor, n=1) -> float:
    """``entropy`` of a real, normalised DiagonalTensor of probabilities (src/tensors/decompositions.cpp:427-450): von
    Neumann ``-sum p log p`` for ``n = 1`` (``p * stable_log(p, 1e-30)`` then the trace, :439-441), ``-log max p`` for
    ``n = inf`` (:444) and the Renyi entropy ``log(sum p^n) / (1 - n)`` otherwise (:446-449).  Each is ONE launch -- the
    ``x log x`` / ``x^n`` pre-map is applied inside the reduction -- and one download of ``16 * n_sectors`` bytes, where the
    reference makes an elementwise pass or two and then a ``sum_all`` per sector."""
    if p.dtype.kind != 'f':
        raise TypeError('entropy: a real DiagonalTensor is required')
    lengths = [int(p.leg.mults[i]) for i in p.block_inds]
    if n == 1:
        table = bb.seg_reduce_many(p.blocks, lengths, 'sum', 'xlogx', 1e-30) if p.blocks else np.zeros((0, 2))
        return -float(sum(_numbers(table, False), 0.0))
    if n == np.inf:
        return -float(np.log(reduce_diagonal(bb, p, 'max')))
    n = float(n)
    table = bb.seg_reduce_many(p.blocks, lengths, 'sum', 'pow', n) if p.blocks else np.zeros((0, 2))
    return float(np.log(sum(_numbers(table, False), 0.0)) / (1.0 - n))
