"""The numpy stand-in of ``tests/numpy_backend.py`` with the grouped entry points the tensor-level operations of
``cyten_amd.abelian`` (conj, dagger, diagonal tensors, scale_axis, partial_trace, dense conversion) call, and with complex
blocks: CPU tests of their HOST logic (test infrastructure)."""
import numpy as np

from numpy_backend import NumpyGroupedBackend
from oracle import block_ops as ops

_UNARY = {'abs': np.abs, 'sqrt': np.sqrt, 'exp': np.exp, 'log': np.log, 'neg': np.negative, 'square': np.square,
          'reciprocal': lambda x: 1.0 / x}
_UNARY_PARAM = {'cutoff_inverse': ops.cutoff_inverse, 'stable_log': ops.stable_log, 'pow': np.power}


class NumpyTensorBackend(NumpyGroupedBackend):
    def as_block(self, a, dtype=None, device=None):
        a = np.asarray(a)
        return np.array(a, dtype=complex if np.iscomplexobj(a) else float)

    def as_complex(self, a):
        return np.asarray(a, dtype=complex)

    def zeros_many(self, shapes, dtype=None, device=None):
        return [np.zeros(sh, dtype=np.dtype(dtype) if dtype is not None else float) for sh in shapes]

    empty_many = zeros_many

    def copy_many(self, pairs, conj=False):
        for d, s in pairs:
            d[...] = np.conj(s) if conj else s

    def norm_many(self, blocks):
        return float(np.sqrt(sum(np.sum(np.abs(b) ** 2) for b in blocks)))

    def scale_axis_many(self, items):
        for _, f, _ in items:
            if np.iscomplexobj(f):
                raise NotImplementedError('complex factors')
        return [ops.scale_axis(a, np.asarray(f), axis) for a, f, axis in items]

    def unary_many(self, blocks, op, param=None):
        if op in _UNARY_PARAM:
            return [_UNARY_PARAM[op](np.asarray(b), param) for b in blocks]
        return [_UNARY[op](np.asarray(b)) for b in blocks]

    def trace_partial_grouped(self, outputs):
        outs = []
        for shape, terms in outputs:
            cplx = any(np.iscomplexobj(t[0]) for t in terms)
            acc = np.zeros(shape, dtype=complex if cplx else float)
            for a, idcs1, idcs2, remaining in terms:
                if a.ndim > 8:
                    raise ValueError('more than 8 axes')
                acc = acc + ops.trace_partial(a, idcs1, idcs2, remaining)
            outs.append(acc)
        return outs
