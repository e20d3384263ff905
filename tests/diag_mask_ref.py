"""numpy side of the tests of the diagonal-tensor arithmetic, reductions and device-side masks of cyten_amd.abelian: the
numpy stand-in backend with the three ``seg_*_many`` entry points, a second stand-in that serves them through a per-block
loop of single-block methods (what the reference's loops issue), and a restatement of each reference function one sector at a
time on plain numpy data, written from the cited lines of src/backends/abelian.cpp and src/tensors/decompositions.cpp."""
import numpy as np

from numpy_tensor_backend import NumpyTensorBackend
from oracle import block_ops as ops

ARITH = {'add': np.add, 'sub': np.subtract, 'mul': np.multiply, 'div': np.divide}
COMPARE = {'lt': np.less, 'le': np.less_equal, 'gt': np.greater, 'ge': np.greater_equal, 'eq': np.equal, 'ne': np.not_equal}
LOGICAL = {'and': np.logical_and, 'or': np.logical_or, 'xor': np.logical_xor}
ALL_BINARY = {**ARITH, **COMPARE, **LOGICAL}


def _num(x):
    """operands of an arithmetic op: booleans count as 0 / 1 (float64), as on the device"""
    x = np.asarray(x)
    return x.astype(float) if x.dtype == bool else x


def block_binary(a, b, op):
    """one block: what ``func(block_a, block_b)`` of the reference gives for the named function"""
    with np.errstate(all='ignore'):
        if op in ARITH:
            return ARITH[op](_num(a), _num(b))
        if op == 'not':
            return np.logical_not(a)
        return ALL_BINARY[op](a, b)


def _pre(x, pre, param):
    with np.errstate(all='ignore'):
        if pre is None:
            return x
        if pre == 'abs':
            return np.abs(x)
        if pre == 'square':
            return x * x
        if pre == 'xlogx':
            return np.where(x > param, x * np.log(np.where(x > param, x, 1.0)), 0.0)
        return np.power(x, param)


def block_reduce(x, op, pre=None, param=None):
    x = _pre(_num(x), pre, param)
    if op == 'count':
        return float(np.count_nonzero(x))
    if op == 'sum':
        return x.sum() if x.size else 0.0
    if x.size == 0:
        return -np.inf if op == 'max' else np.inf
    return float(x.max() if op == 'max' else x.min())


class _Base(NumpyTensorBackend):
    """what both stand-ins share: boolean blocks, diagonal views, index tables as gather / scatter arguments"""

    def as_block(self, a, dtype=None, device=None):
        a = np.asarray(a)
        return a.copy() if a.dtype == bool else super().as_block(a)

    def is_correct_block_type(self, b):
        return isinstance(b, np.ndarray)

    def diagonal_view(self, a):
        return np.einsum('ii->i', a)

    def off_diagonal_view(self, a):
        n = a.shape[0]
        return a.reshape(-1)[1:].reshape(n - 1, n + 1)[:, :n] if n > 1 else np.zeros((0, n), a.dtype)

    def max_abs_many(self, blocks):
        return max([float(np.abs(b).max()) for b in blocks if b.size], default=0.0)

    def mask_gather_many(self, items):
        return [np.compress(m, a, ax) if np.asarray(m).dtype == bool else np.take(a, np.asarray(m, dtype=np.int64), ax) for a, m, ax in items]

    def enlarge_leg_many(self, items):
        outs = []
        for a, m, ax in items:
            if isinstance(m, tuple):
                flags = np.zeros(int(m[1]), dtype=bool)
                flags[np.asarray(m[0], dtype=np.int64)] = True
                m = flags
            outs.append(ops.enlarge_leg(a, np.asarray(m, dtype=bool), ax))
        return outs


class NumpySegmentBackend(_Base):
    """the grouped entry points, each over the whole list at once"""

    def __init__(self):
        self.calls = []

    def seg_binary_many(self, items, op, scalar=None, complex_out=False):
        self.calls.append(('seg_binary_many', len(items)))
        cplx = any(np.iscomplexobj(x) for a, b, _ in items for x in (a, b) if x is not None) or np.iscomplexobj(scalar) or complex_out
        outs = []
        for a, b, n in items:
            a = np.zeros(n) if a is None else a
            b = scalar if scalar is not None else (np.zeros(n) if b is None else b)
            if op in LOGICAL or op == 'not':
                a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
            r = block_binary(a, b, op)
            outs.append(r.astype(complex) if cplx and op in ARITH else r)
        return outs

    def seg_reduce_many(self, blocks, lengths, op, pre=None, param=None):
        self.calls.append(('seg_reduce_many', len(blocks)))
        table = np.zeros((len(blocks), 2))
        for s, (b, n) in enumerate(zip(blocks, lengths)):
            v = block_reduce(np.zeros(n) if b is None else b, op, pre, param)
            table[s] = (np.real(v), np.imag(v))
        return table

    def seg_compact_many(self, flag_blocks):
        self.calls.append(('seg_compact_many', len(flag_blocks)))
        tables = [np.flatnonzero(b).astype(np.int64) for b in flag_blocks]
        return tables, np.array([len(t) for t in tables], dtype=np.int64)


class NumpyBlockLoopBackend(_Base):
    """the same three entry points served by a per-block loop of single-block methods, zero blocks for the missing sectors
    included: the sequence of calls the reference's per-sector loops make (abelian.cpp:1596-1619, :1707-1728, :2410-2440,
    :3163-3173)"""

    def zeros(self, shape, dtype=None, device=None):
        return np.zeros(shape, dtype=dtype or float)

    def sum_all(self, a):
        return _num(a).sum()

    def any(self, a):
        return bool(np.any(a))

    def max(self, a):
        return float(np.max(a))

    def min(self, a):
        return float(np.min(a))

    def seg_binary_many(self, items, op, scalar=None, complex_out=False):
        cplx = any(np.iscomplexobj(x) for a, b, _ in items for x in (a, b) if x is not None) or np.iscomplexobj(scalar) or complex_out
        logical = op in LOGICAL or op == 'not'
        outs = []
        for a, b, n in items:
            a = self.zeros((n,), bool if logical else None) if a is None else a
            b = scalar if scalar is not None else (self.zeros((n,), bool if logical else None) if b is None else b)
            r = block_binary(a, b, op)
            outs.append(self.to_dtype(r, complex) if cplx and op in ARITH else r)
        return outs

    def seg_reduce_many(self, blocks, lengths, op, pre=None, param=None):
        table = np.zeros((len(blocks), 2))
        for s, (b, n) in enumerate(zip(blocks, lengths)):
            b = _pre(_num(self.zeros((n,)) if b is None else b), pre, param)
            if op == 'count':
                v = self.sum_all(b != 0)
            elif op == 'sum':
                v = self.sum_all(b)
            elif n == 0:
                v = -np.inf if op == 'max' else np.inf
            else:
                v = self.max(b) if op == 'max' else self.min(b)
            table[s] = (np.real(v), np.imag(v))
        return table

    def seg_compact_many(self, flag_blocks):
        tables, counts = [], []
        for b in flag_blocks:
            flags = self.to_numpy(b) != 0
            counts.append(int(self.sum_all(flags)) if self.any(flags) else 0)
            tables.append(np.flatnonzero(flags).astype(np.int64))
        return tables, np.array(counts, dtype=np.int64)


# ------------------------------------------------------------------------------------------- the reference, restated
# A diagonal is (inds, blocks): ascending sector indices and one numpy vector per index.  `mults`: the leg.

def ref_diagonal_binary(mults, a, b, op, partial_zero_is_zero, dtype_a=float, dtype_b=float):
    """abelian.cpp:1596-1631"""
    (a_inds, a_blocks), (b_inds, b_blocks) = a, b
    ia = ib = 0
    blocks, inds = [], []
    for i in range(len(mults)):
        if ia < len(a_inds) and a_inds[ia] == i:
            block_a = a_blocks[ia]
            ia += 1
        elif partial_zero_is_zero:
            # The reference `continue`s here without stepping over a block of b in this sector (:1602-1603), after which its
            # `bi_b` never matches again and every later block of b counts as missing.  The rule it states -- a sector missing on
            # either side is skipped -- is what is restated (and built) here.
            if ib < len(b_inds) and b_inds[ib] == i:
                ib += 1
            continue
        else:
            block_a = np.zeros(mults[i], dtype=dtype_a)
        if ib < len(b_inds) and b_inds[ib] == i:
            block_b = b_blocks[ib]
            ib += 1
        elif partial_zero_is_zero:
            continue
        else:
            block_b = np.zeros(mults[i], dtype=dtype_a)
        blocks.append(block_binary(block_a, block_b, op))
        inds.append(i)
    if blocks:
        dtype = blocks[0].dtype
    else:
        dtype = block_binary(np.ones(1, dtype=dtype_a), np.ones(1, dtype=dtype_b), op).dtype    # the sample rule, :1622-1626
    return inds, blocks, np.dtype(dtype)


def dense_of(mults, diag, dtype=None):
    """abelian.cpp:1679-1692"""
    inds, blocks = diag
    sl = np.concatenate([[0], np.cumsum(mults)])
    if dtype is None:
        dtype = np.result_type(*[b.dtype for b in blocks]) if blocks else float
    out = np.zeros(int(sl[-1]), dtype=dtype)
    for i, b in zip(inds, blocks):
        out[sl[i]:sl[i + 1]] = b
    return out


def ref_all(mults, diag):
    """abelian.cpp:717-730"""
    inds, blocks = diag
    if len(inds) < len(mults):
        return False
    return all(bool(np.all(b)) for b in blocks)


def ref_any(diag):
    """abelian.cpp:733-740"""
    return any(bool(np.any(b)) for b in diag[1])


def ref_reduce(mults, diag, block_func, func, dtype=float):
    """abelian.cpp:3154-3175"""
    inds, blocks = diag
    numbers, i = [], 0
    for j in range(len(mults)):
        if i < len(inds) and inds[i] == j:
            block = blocks[i]
            i += 1
        else:
            block = np.zeros(mults[j], dtype=dtype)
        numbers.append(block_func(block))
    return func(numbers)


def ref_trace(diag, dtype=float):
    """abelian.cpp:966-973"""
    total = np.dtype(dtype).type(0)
    for b in diag[1]:
        total = total + b.sum()
    return total


def ref_to_mask(mults, diag):
    """abelian.cpp:1707-1755 without a basis permutation: (large sector indices of the kept blocks, their flag blocks,
    multiplicities of the small leg)"""
    inds, blocks = diag
    large, flags, small_mults = [], [], []
    for bii, blk in zip(inds, blocks):
        if not np.any(blk):
            continue
        flags.append(blk)
        large.append(bii)
        small_mults.append(int(blk.sum()))
    return large, flags, small_mults


def ref_mask_binary(mults, m1, m2, op):
    """abelian.cpp:2410-2440 (m2 = None: mask_unary_operand with logical_not, :2705-2728).  A mask is (large sector indices,
    flag blocks)."""
    i1 = i2 = 0
    large, flags, small_mults = [], [], []
    for s in range(len(mults)):
        if i1 < len(m1[0]) and m1[0][i1] == s:
            b1 = m1[1][i1]
            i1 += 1
        else:
            b1 = np.zeros(mults[s], dtype=bool)
        if m2 is None:
            new = np.logical_not(b1)
        else:
            if i2 < len(m2[0]) and m2[0][i2] == s:
                b2 = m2[1][i2]
                i2 += 1
            else:
                b2 = np.zeros(mults[s], dtype=bool)
            new = LOGICAL[op](b1, b2)
        mult = int(new.sum())
        if mult == 0:
            continue
        flags.append(new)
        large.append(s)
        small_mults.append(mult)
    return large, flags, small_mults


def ref_apply_mask(diag, mask):
    """abelian.cpp:646-673: the common sectors, ``apply_mask`` each, the block index is the one on the small leg"""
    (inds, blocks), (large, flags) = diag, mask
    out_inds, out_blocks = [], []
    for j, (s, f) in enumerate(zip(large, flags)):
        if s in inds:
            out_blocks.append(blocks[list(inds).index(s)][f])
            out_inds.append(j)
    return out_inds, out_blocks


def ref_entropy(p, n=1):
    """the sequence-of-floats branch, decompositions.cpp:452-463"""
    p = np.real_if_close(np.asarray(p))
    p = p[p > 1e-30]
    if n == 1:
        return -np.inner(np.log(p), p)
    if n == np.inf:
        return -np.log(np.max(p))
    return np.log(np.sum(p ** n)) / (1.0 - n)
