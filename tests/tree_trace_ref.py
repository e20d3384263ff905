"""numpy restatement of step 2 of ``FusionTreeBackend::partial_trace`` (src/backends/fusion_tree_backend.cpp:3092-3159), one
tree pair at a time with the block-backend calls the reference makes, on the data structures of ``cyten_amd.fusion_tree``
(TreeSpace, FusionTreeData with numpy blocks, TreeTrace tables).  Kept apart from the code under test: it shares only the
containers with it."""
import numpy as np

from cyten_amd import fusion_tree as ft


def trace_partial(a, idcs1, idcs2, remaining):
    """NumpyBlockBackend::trace_partial (src/block_backend/numpy.cpp:1166-1195): transpose to remaining + idcs1 + idcs2, fuse
    each group into one axis of extent T, trace over the last two axes"""
    t = np.transpose(a, list(remaining) + list(idcs1) + list(idcs2))
    T = int(np.prod([a.shape[i] for i in idcs1], dtype=np.int64))
    rshape = [a.shape[i] for i in remaining]
    return np.trace(t.reshape(rshape + [T, T]), axis1=-2, axis2=-1)


def _lookup(trace, tree):
    """partial_trace_helper (:2557-2604) as data: (on_diag, factor, new tree)"""
    if trace is None:
        return True, 1.0, tree
    hit = trace.table.get(tree)
    return (False, 0.0, None) if hit is None else (True, hit[1], hit[0])


def partial_trace_ref(data, codomain, domain, new_codomain, new_domain, cod_trace=None, dom_trace=None, eps=0.0, absolute=False,
                      count=False):
    """{(i_new, j_new): block} of the traced tensor.  ``absolute``: data and factors are replaced by |re| + |im| (the S of an
    error bound); ``count``: by ones (the number of addends N of every element)."""
    def val(x):
        x = np.asarray(x)
        if count:
            return np.ones(x.shape)
        return np.abs(x.real) + np.abs(x.imag) if absolute else x

    J = codomain.num_legs
    tr1 = list(cod_trace.positions if cod_trace else ()) + [J + k for k in (dom_trace.positions if dom_trace else ())]
    tr2 = [k + 1 for k in tr1]
    remain = [k for k in range(J + domain.num_legs) if k not in tr1 and k not in tr2]
    blocks = [val(b) for b in data.blocks]
    factors = [f for tr in (cod_trace, dom_trace) if tr for _, f in tr.table.values()]
    cplx = not (absolute or count) and (any(np.iscomplexobj(b) for b in blocks) or any(complex(f).imag != 0 for f in factors))
    # :3027-3047: coupled sectors of the data that both new spaces hold; :3037: zero blocks for every common sector
    new = {(i, j): np.zeros((new_codomain.block_size(i), new_domain.block_size(j)), dtype=complex if cplx else float)
           for i, j in ft.common_sectors(new_codomain, new_domain)}
    where_c = {tuple(s): k for k, s in enumerate(new_codomain.sectors.tolist())}
    where_d = {tuple(s): k for k, s in enumerate(new_domain.sectors.tolist())}
    touched = set()
    for n, (i_old, j_old) in enumerate(data.block_inds.tolist()):
        sector = tuple(domain.sectors[j_old].tolist())
        if sector not in where_d or sector not in where_c:
            continue                                                                          # :3031-3034
        key = (where_c[sector], where_d[sector])
        touched.add(key)
        for cod_tb in codomain.tree_blocks[i_old]:                                            # :3092
            on_diag, f_cod, new_cod_tree = _lookup(cod_trace, cod_tb.tree)                    # :3093
            if not on_diag:
                continue                                                                      # :3094-3095
            _, new_cod = new_codomain.tree_block_slice(new_cod_tree)                          # :3109-3110
            for dom_tb in domain.tree_blocks[j_old]:                                          # :3116-3117
                on_diag2, f_dom, new_dom_tree = _lookup(dom_trace, dom_tb.tree)               # :3118
                if not on_diag2:
                    continue                                                                  # :3119-3120
                tmp_shape = list(cod_tb.multiplicities) + list(dom_tb.multiplicities)         # :3121-3123
                _, new_dom = new_domain.tree_block_slice(new_dom_tree)                        # :3136-3137
                old_block = blocks[n][cod_tb.start:cod_tb.stop, dom_tb.start:dom_tb.stop]     # :3139-3141
                old_block = old_block.reshape(tmp_shape)                                      # :3142
                contribution = trace_partial(old_block, tr1, tr2, remain)                     # :3143-3144
                contribution = contribution.reshape(new_cod.stop - new_cod.start, new_dom.stop - new_dom.start)   # :3145-3147
                factor = f_cod * np.conj(f_dom)                                               # :3148-3149
                if absolute or count:
                    factor = float(val(factor))
                contribution = factor * contribution                                          # :3150
                cur = new[key][new_cod.start:new_cod.stop, new_dom.start:new_dom.stop]        # :3151-3153
                new[key][new_cod.start:new_cod.stop, new_dom.start:new_dom.stop] = cur + contribution             # :3154-3157
    scalar = new_codomain.num_legs == 0 and new_domain.num_legs == 0
    if scalar or absolute or count:
        return new if scalar else {k: b for k, b in new.items() if k in touched}              # (:3162-3181: the scalar block stays)
    return {k: b for k, b in new.items() if np.abs(b).max(initial=0.0) > eps}                 # :3160 discard_zero_blocks
