"""Deferred execution behind the reference's ONE-BLOCK-AT-A-TIME call sites (route 1).

cyten's tensor backends call the block backend per block: the hot loop of a contraction is

    block = bb.matrix_dot(a, b)
    block = block + bb.matrix_dot(a', b')        # Block::operator+  (abelian.cpp:1437-1446)
    res_blocks.append(bb.reshape(block, shape))  #                   (abelian.cpp:1455-1459)

and nothing looks at the data until much later.  :class:`DeferredBlockBackend` serves exactly these calls without
launching anything: ``matrix_dot`` returns a :class:`LazyBlock` whose shape / dtype / device are known and whose
data is a pending GEMM node, ``+`` of two pending nodes appends a K-segment, ``reshape`` / ``permute_axes`` of a
pending node stay metadata.  The queue is flushed as ONE grouped launch (``cyb_gemm_grouped_enqueue_f64``) the
first time anything needs the values (``to_numpy``, any kernel that reads the block, ``synchronize`` ...): the
reference's ``synchronize()`` is an empty non-virtual (block_backend.cpp:1042-1045), so flushing on observation is
the only correct trigger.  The per-sector decomposition loops (``bb.matrix_svd(block)`` per coupled charge,
abelian.cpp:3499-3541; likewise ``matrix_qr`` / ``eigh``) are deferred the same way: the three results of a
pending SVD are lazy blocks of known shape, and the first observation -- ``truncate_singular_values`` reading S
(abelian.cpp:3631) -- runs ALL pending decompositions as one batched call.  Everything else is inherited from
:class:`HipBlockBackend` unchanged.
"""
from __future__ import annotations

import numpy as np

from .block_backend import HipBlock, HipBlockBackend


class LazyBlock(HipBlock):
    """A block whose data is a pending sum of matrix products -- or a ``reshape`` / ``permute_axes`` VIEW of one (``_base``
    is the product node, ``_view_ops`` the chain of metadata operations from it).  Reading ``buf`` / ``offset`` /
    ``strides`` (i.e. handing the block to any kernel) materialises the whole queue of its backend.  Nodes are never
    dropped: a product that was folded into a longer K-segment chain by ``+`` leaves the queue, but can still be
    materialised on its own if somebody reads it later."""

    __slots__ = ('_segments', '_view_ops', '_real', '_cplx', '_base', '_queued')

    def __init__(self, backend, shape, segments, cplx, base=None, view_ops=()):
        # (HipBlock.__init__ is bypassed on purpose: buf / offset / strides are properties here)
        object.__setattr__(self, 'backend', backend)
        object.__setattr__(self, 'shape', tuple(int(s) for s in shape))
        self._segments = segments     # [(a, b)] 2-D operands; result = sum a @ b  (product nodes)
        self._base = base             # the product node this is a view of (None: this IS a product node)
        self._view_ops = list(view_ops)   # [('reshape', shape) | ('permute', perm)] applied to the base's result
        self._real = None
        self._cplx = cplx
        self._queued = base is None

    @property
    def _root(self):
        return self._base if self._base is not None else self

    def _resolved(self) -> bool:
        return self._root._real is not None

    def _force(self) -> HipBlock:
        if self._real is None:
            bb = self.backend
            if self._base is not None:
                blk = self._base._force()
                for op, arg in self._view_ops:
                    blk = HipBlockBackend.reshape(bb, blk, arg) if op == 'reshape' else HipBlockBackend.permute_axes(bb, blk, arg)
                self._real = blk
            elif self._queued:
                bb.flush()
                if self._real is None:   # still pending: an operand is the output of a decomposition that failed
                    raise RuntimeError('deferred queue: an operand of this product comes from a decomposition that failed')
            else:   # an addend that was folded into a longer chain and is read after all: its own launch
                bb._run_products([self])
        return self._real

    buf = property(lambda self: self._force().buf)
    offset = property(lambda self: self._force().offset)
    strides = property(lambda self: self._force().strides)
    ptr = property(lambda self: self._force().ptr)   # (HipBlock caches address and contiguity per view: ask the real one)

    @property
    def is_complex(self):
        return self._cplx

    @property
    def dtype(self):
        return np.dtype('complex128') if self._cplx else np.dtype('float64')

    def is_contiguous(self):
        return self._force().is_contiguous()

    def __add__(self, other):
        if (isinstance(other, LazyBlock) and other._real is None and self._real is None and self._base is None
                and other._base is None and self._queued and other._queued and other.shape == self.shape
                and other.backend is self.backend):
            # Block::operator+ of two pending products: one more K-segment, still nothing launched
            merged = LazyBlock(self.backend, self.shape, self._segments + other._segments, self._cplx or other._cplx)
            self.backend._fold_pending([self, other], merged)
            return merged
        return HipBlock.__add__(self, other)

    def __repr__(self):
        state = 'pending' if self._real is None else 'materialised'
        kind = f'view of {len(self._root._segments)}-segment product' if self._base is not None else f'{len(self._segments)} segment(s)'
        return f'LazyBlock(shape={self.shape}, {kind}, {state})'


class _DecompNode:
    """A pending decomposition of one block: kind 'svd' | 'qr' | 'eigh', its argument(s) and lazy outputs."""

    def __init__(self, kind, block, arg):
        self.kind, self.block, self.arg, self.outs = kind, block, arg, []
        self.error = None   # the LinAlgError of a run that failed: the node has left the queue, forcing an output runs it again


class LazyOut(HipBlock):
    """One output of a pending decomposition (shape known up front, data after the batched call)."""

    __slots__ = ('_node', '_real')

    def __init__(self, backend, shape, node):
        object.__setattr__(self, 'backend', backend)
        object.__setattr__(self, 'shape', tuple(int(s) for s in shape))
        self._node = node
        self._real = None

    def _force(self) -> HipBlock:
        if self._real is None:
            node = self._node
            if node.error is None:
                self.backend.flush()
                if self._real is None and node.error is not None:
                    raise node.error
                if self._real is None:   # still pending: its input waits for the output of a decomposition that failed
                    raise RuntimeError('deferred queue: the input of this decomposition comes from a decomposition that failed')
            else:   # failed in an earlier flush and left the queue: only its own outputs run it again (and raise again)
                self.backend._retry_decomp(node)
        return self._real

    buf = property(lambda self: self._force().buf)
    offset = property(lambda self: self._force().offset)
    strides = property(lambda self: self._force().strides)
    ptr = property(lambda self: self._force().ptr)
    is_complex = property(lambda self: False)
    dtype = property(lambda self: np.dtype('float64'))

    def is_contiguous(self):
        return self._force().is_contiguous()


class DeferredBlockBackend(HipBlockBackend):
    """HipBlockBackend whose ``matrix_dot`` is lazy (see the module docstring)."""

    def __init__(self, default_device: str = 'cuda:0'):
        super().__init__(default_device)
        self._pending = []
        self._pending_decomp = []
        self._flushing = False
        self.n_flushes = 0          # grouped launches issued by flush() (tests read this)
        self.n_deferred = 0         # matrix_dot calls served lazily
        self.n_decomp_batches = 0   # batched decomposition calls issued by flush()

    # a lazy block has no address and no strides until it is flushed: combine_legs / split_legs take the generic
    # zeros_many + copy_many route with this backend instead of a placement plan
    place_plan = None

    # ---- the lazy producer
    def matrix_dot(self, a: HipBlock, b: HipBlock) -> HipBlock:
        if a.ndim != 2 or b.ndim != 2:
            return super().matrix_dot(a, b)
        if a.shape[1] != b.shape[0]:
            raise ValueError(f'shapes {a.shape} and {b.shape} not aligned')
        node = LazyBlock(self, (a.shape[0], b.shape[1]), [(a, b)], a.is_complex or b.is_complex)
        self._pending.append(node)
        self.n_deferred += 1
        return node

    # ---- lazy decompositions (one block per call in the reference, one batched call here)
    def _defer_decomp(self, kind, a, arg, shapes):
        if a.ndim != 2:
            raise ValueError(f'{kind}: block must be 2-D')
        if a.is_complex:  # lazy outputs are typed float64: complex blocks are decomposed at once (their own batched call)
            self.flush()
            if kind == 'svd':
                return list(HipBlockBackend.matrix_svd_batched(self, [a], arg)[0])
            if kind == 'qr':
                return list(HipBlockBackend.matrix_qr_batched(self, [a], arg)[0])
            return list(HipBlockBackend.eigh_batched(self, [a], arg)[0])
        node = _DecompNode(kind, a, arg)
        node.outs = [LazyOut(self, shp, node) for shp in shapes]
        self._pending_decomp.append(node)
        return node.outs

    def matrix_svd(self, a, algorithm=None):
        if algorithm is not None and algorithm not in self.svd_algorithms:
            raise ValueError(f'SVD algorithm not supported: {algorithm}')
        m, n = a.shape
        k = min(m, n)
        return tuple(self._defer_decomp('svd', a, algorithm, [(m, k), (k,), (k, n)]))

    def matrix_qr(self, a, full: bool):
        m, n = a.shape
        kq = m if full else min(m, n)
        return tuple(self._defer_decomp('qr', a, bool(full), [(m, kq), (kq, n)]))

    def eigh(self, block, sort=None):
        n = block.shape[0]
        return tuple(self._defer_decomp('eigh', block, sort, [(n,), (n, n)]))

    def _fold_pending(self, old, new):
        """`old` products were summed into `new` (one more K-segment): they leave the queue but stay materialisable."""
        ids = {id(o) for o in old}
        self._pending = [p for p in self._pending if id(p) not in ids]
        for o in old:
            o._queued = False
        self._pending.append(new)

    # ---- metadata-only consumers keep the node pending
    def reshape(self, a, shape):
        if isinstance(a, LazyBlock) and a._real is None:
            shape = [int(s) for s in shape]
            if -1 in shape:
                known = int(np.prod([s for s in shape if s != -1], dtype=np.int64))
                shape[shape.index(-1)] = a.size // max(known, 1)
            if int(np.prod(shape, dtype=np.int64)) != a.size:
                raise ValueError(f'cannot reshape block of size {a.size} into {shape}')
            return LazyBlock(self, shape, a._root._segments, a._cplx, base=a._root,
                             view_ops=a._view_ops + [('reshape', tuple(shape))])
        return super().reshape(a, shape)

    def permute_axes(self, a, permutation):
        if isinstance(a, LazyBlock) and a._real is None:
            perm = [int(p) for p in permutation]
            return LazyBlock(self, [a.shape[p] for p in perm], a._root._segments, a._cplx, base=a._root,
                             view_ops=a._view_ops + [('permute', tuple(perm))])
        return super().permute_axes(a, permutation)

    # ---- the flush: grouped launches for everything that is pending, in dependency order
    @staticmethod
    def _is_resolved(x) -> bool:
        if isinstance(x, LazyBlock):
            return x._resolved()
        if isinstance(x, LazyOut):
            return x._real is not None
        return True

    def _run_products(self, batch):
        outs = HipBlockBackend.matrix_dot_grouped(self, [p._segments for p in batch])
        self.n_flushes += 1
        for p, out in zip(batch, outs):
            p._real = out

    def _run_decomps(self, nodes):
        for kind in ('svd', 'qr', 'eigh'):
            for arg in {n.arg for n in nodes if n.kind == kind}:  # one batched call per (kind, option)
                sel = [n for n in nodes if n.kind == kind and n.arg == arg]
                blocks = [n.block for n in sel]
                if kind == 'svd':
                    res = HipBlockBackend.matrix_svd_batched(self, blocks, arg)
                elif kind == 'qr':
                    res = HipBlockBackend.matrix_qr_batched(self, blocks, arg)
                else:
                    res = HipBlockBackend.eigh_batched(self, blocks, arg)
                self.n_decomp_batches += 1
                for n, outs in zip(sel, res):
                    for lazy, real in zip(n.outs, outs):
                        lazy._real = real

    def _run_decomps_isolating(self, nodes):
        """``_run_decomps`` with a LinAlgError confined to the blocks that cause it: a batched call that raises is repeated
        block by block, and a block that fails alone keeps the exception on its node and leaves the queue -- forcing one of
        its outputs raises it (``LazyOut._force``), nothing else does."""
        from ._lib import LinAlgError
        try:
            self._run_decomps(nodes)
            return
        except LinAlgError as exc:
            if len(nodes) == 1:
                nodes[0].error = exc
                return
        for n in nodes:
            if all(o._real is not None for o in n.outs):
                continue
            try:
                self._run_decomps([n])
            except LinAlgError as exc:
                n.error = exc

    def _retry_decomp(self, node):
        """a node that failed before, on behalf of one of its outputs: alone, after whatever its input still waits for"""
        if not self._is_resolved(node.block):
            self.flush()
        self._run_decomps([node])   # (raises again if the block is still bad)
        node.error = None

    @classmethod
    def _blocked(cls, x) -> bool:
        """does `x` wait for the output of a decomposition that failed?"""
        if isinstance(x, LazyOut):   # of a node that failed, or of one whose own input waits for such a node
            return x._real is None and (x._node.error is not None or cls._blocked(x._node.block))
        if isinstance(x, LazyBlock):
            root = x._root
            return root._real is None and any(cls._blocked(y) for seg in root._segments for y in seg)
        return False

    def flush(self):
        """Topological rounds over BOTH kinds of pending work: every product whose operands exist runs in one grouped
        launch, then every decomposition whose input exists runs in one batched call per kind, and so on -- a chain
        ``matrix_dot -> matrix_qr of that product -> matrix_dot with Q`` (tdot -> qr -> tdot on 2-leg tensors) needs three
        rounds, the reference's contraction / SVD loops one each.  No nested flush: operands are only marshalled once
        everything they depend on has been materialised.  A block without a decomposition (LinAlgError: NaN entries, no
        convergence) does not make flush() raise: the error stays with that block's outputs, the other blocks of its batch
        are decomposed one by one, and work that depends on the failed outputs stays queued."""
        if self._flushing:
            raise RuntimeError('deferred queue: flush() re-entered (an operand was read before its producer ran)')
        self._flushing = True
        products, self._pending = [p for p in self._pending if p._real is None], []
        decomps, self._pending_decomp = self._pending_decomp, []
        stalled_p, stalled_d = [], []   # work behind a failed decomposition: stays queued, runs once a retry of that node succeeds
        try:
            while products or decomps:
                batch = [p for p in products if all(self._is_resolved(x) for seg in p._segments for x in seg)]
                if batch:
                    ids = {id(p) for p in batch}
                    self._run_products(batch)
                    products = [p for p in products if id(p) not in ids]
                    continue
                ready = [n for n in decomps if self._is_resolved(n.block)]
                if ready:
                    ids = {id(n) for n in ready}
                    decomps = [n for n in decomps if id(n) not in ids]
                    try:
                        self._run_decomps_isolating(ready)
                    except BaseException:
                        decomps = ready + decomps
                        raise
                    continue
                # nothing is ready: an operand may be an addend that `+` folded into a longer chain (it left the queue, so no
                # round above will ever produce it) -- or a view of one.  Run those products on their own, then look again.
                orphans = {}
                for x in [x for p in products for seg in p._segments for x in seg] + [n.block for n in decomps]:
                    root = x._root if isinstance(x, LazyBlock) else None
                    if root is not None and root._real is None and not root._queued and all(
                            self._is_resolved(y) for seg in root._segments for y in seg):
                        orphans[id(root)] = root
                if orphans:
                    self._run_products(list(orphans.values()))
                    continue
                held_p = [p for p in products if self._blocked(p)]
                held_d = [n for n in decomps if self._blocked(n.block)]
                if held_p or held_d:
                    ids = {id(x) for x in held_p + held_d}
                    stalled_p += held_p
                    stalled_d += held_d
                    products = [p for p in products if id(p) not in ids]
                    decomps = [n for n in decomps if id(n) not in ids]
                    continue
                raise RuntimeError('deferred queue: cyclic dependency between pending products / decompositions')
        except BaseException:
            # a launch failed for another reason than a block without a decomposition (a HIP error, an interrupt): what has not
            # run goes back on the queues, so that the surviving lazy blocks stay materialisable instead of reading None
            self._pending = [p for p in products if p._real is None] + self._pending
            self._pending_decomp = [n for n in decomps if n.error is None and any(o._real is None for o in n.outs)] + self._pending_decomp
            raise
        finally:
            self._pending = stalled_p + self._pending
            self._pending_decomp = stalled_d + self._pending_decomp
            self._flushing = False

    def synchronize(self):
        self.flush()
        super().synchronize()
