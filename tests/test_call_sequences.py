"""The descriptor-ring rule of cyb_ctx_s::upload restated and checked as a model, and the call lists of
call_sequence_cases.py checked against their own conditions, so that the GPU run of them (test_gpu_call_sequences.py) cannot
be vacuous.  No device is needed."""
import ctypes as C
import os
import re

import numpy as np

import call_sequence_cases as cs
from cyten_amd import _lib

K = cs.ring_constants()


def test_constants_are_read_from_the_header():
    assert all(v > 0 for v in K.values()) and K['kBig'] % 2 == 0 and K['kSlots'] % 2 == 0
    assert K['kSlots'] // 2 > K['kEvStride']          # the static_assert of upload()
    assert K['kSlots'] % K['kEvStride'] == 0          # an event lives in the slot of the upload that recorded it


def test_model_formulas_restate_upload():
    """waited_event / waited_event_big are the index arithmetic of cyb_ctx_s::upload (api.hip), line for line"""
    src = open(os.path.join(cs.ROOT, 'cyten_amd', 'csrc', 'api.hip')).read()
    # small ring: slot, the threshold, the awaited event, where events are recorded
    assert 'Slot& s = slots[j % kSlots];' in src
    assert re.search(r'if \(j >= \(uint64_t\)kSlots\) \{\s*const uint64_t e = \(j - kSlots / 2 \+ kEvStride - 1\) / kEvStride \* kEvStride;', src)
    assert 'Slot& w = slots[e % kSlots];' in src and 'if (j % kEvStride == 0) {' in src
    # big ring: slot, the threshold, the awaited event; an event with every big upload
    assert 'Slot& b = big[jb % kBig];' in src
    assert re.search(r'if \(jb >= \(uint64_t\)kBig\) \{\s*Slot& w = big\[\(jb - kBig / 2\) % kBig\];', src)
    assert re.search(r'CYB_HIP\(hipEventRecord\(b\.ev, stream\)\);\s*b\.ev_valid = true;', src)
    assert 'if (bytes > kBigBytes) {' in src
    ks, st, kb = 32, 8, 8
    for j in (0, 31, 32, 40, 41, 48, 1000):
        want = None if j < ks else (j - ks // 2 + st - 1) // st * st
        assert cs.waited_event(j, ks, st) == want
        assert cs.waited_event_big(j, kb) == (None if j < kb else j - kb // 2)


def test_small_ring_model():
    """Replay of upload() for 4 kSlots kEvStride uploads.  Upload j refills slot j % kSlots, last filled by upload
    u = j - kSlots, after waiting for the event recorded at the start of upload e(j).  A consumer of upload u that is launched
    before upload e(j) starts is therefore finished when the slot is overwritten; one launched later is not covered.  The
    number of further uploads a call may make between filling a slot and launching its consumer is e(j) - u - 1, and the
    smallest value over j is the contract."""
    ks, st = K['kSlots'], K['kEvStride']
    recorded_at = {}        # event index -> upload during which it was recorded
    filled_at = {}          # slot -> upload that filled it last
    allowed = []
    for j in range(4 * ks * st):
        e = cs.waited_event(j, ks, st)
        if j < ks:
            assert e is None and (j % ks) not in filled_at            # a fresh slot: nothing to wait for
        else:
            assert e in recorded_at and recorded_at[e] == e < j      # recorded before upload j
            assert e >= j - ks // 2                                   # ... and no earlier than upload j - kSlots/2
            assert filled_at[e % ks] == e                             # the event still sits in its slot: that slot was not refilled
            u = filled_at[j % ks]
            assert u == j - ks and u < e                              # the slot was last filled before e
            allowed.append(e - u - 1)
        if j % st == 0:
            recorded_at[j] = j
        filled_at[j % ks] = j
    assert min(allowed) == ks // 2 - 1 and max(allowed) == ks // 2 - 1 + st - 1
    # jacobi_engine.hip keeps a cached image alive while fewer than kSlots/2 - 1 uploads were made since the one that filled it
    # (cached_at is n_uploads AFTER that upload): at most kSlots/2 - 2 further uploads, inside the rule
    src = open(os.path.join(cs.ROOT, 'cyten_amd', 'csrc', 'jacobi_engine.hip')).read()
    assert re.search(r'ctx->n_uploads - cached_at < \(uint64_t\)cyb_ctx_s::kSlots / 2 - 1', src)
    assert re.search(r'cached_at = ctx->n_uploads;', src)
    assert (ks // 2 - 1) - 1 <= min(allowed)


def test_big_ring_model():
    """the same for the ring of images above kBigBytes: every big upload records an event, upload j waits for that of j - kBig/2"""
    kb = K['kBig']
    filled_at, allowed = {}, []
    for j in range(16 * kb):
        e = cs.waited_event_big(j, kb)
        if j < kb:
            assert e is None
        else:
            assert e < j and e >= j - kb // 2 and filled_at[e % kb] == e
            u = filled_at[j % kb]
            assert u == j - kb and u < e
            allowed.append(e - u - 1)
        filled_at[j % kb] = j
    assert set(allowed) == {kb // 2 - 1}


def test_gate_points_keep_a_gate_younger_than_every_awaited_event():
    """gate_points(): whatever event an upload of the sequence waits for, a gate was queued after that event was recorded and
    before the waiting upload -- for every ring phase the GPU test starts from"""
    ks, st, kb = K['kSlots'], K['kEvStride'], K['kBig']
    for calls in (cs.small_ring_sequence(), cs.big_ring_sequence()):
        for phase in (0, 5, 13):
            gates = set(cs.gate_points(calls, K))
            j, jb, last_gate_small, last_gate_big = phase, 0, -1, -1
            for i, c in enumerate(calls):
                if i in gates:
                    last_gate_small, last_gate_big = j, jb      # queued before uploads j (small) / jb (big)
                for _ in range(c.uploads):
                    e = cs.waited_event(j, ks, st)
                    assert e is None or last_gate_small > e
                    j += 1
                for _ in range(c.big_uploads):
                    e = cs.waited_event_big(jb, kb)
                    assert e is None or last_gate_big > e
                    jb += 1


def _check_reference_shapes(calls):
    for c in calls:
        assert hasattr(_lib, 'PROTOTYPES') and c.entry in _lib.PROTOTYPES
        assert set(c.expected) <= set(c.outputs) and set(c.tol) == set(c.expected)
        for name, want in c.expected.items():
            assert want.shape == c.outputs[name].shape and want.dtype == c.outputs[name].dtype, (c.entry, name)
            assert np.all(np.isfinite(want.view(np.float64) if want.dtype.kind == 'c' else want.astype(np.float64)))
            assert np.all(np.asarray(c.tol[name]) >= 0)


def test_small_ring_sequence_meets_its_conditions():
    calls = cs.small_ring_sequence()
    small, big = cs.count_uploads(calls)
    assert big == 0 and small >= 80 and small >= 2 * K['kSlots'] + 13        # every slot refilled twice, from every start offset
    assert sum(1 for c in calls if c.uploads == 1) >= 80
    wanted = {'cyb_copy_strided_batched', 'cyb_binary_batched_f64', 'cyb_axpby_batched_f64', 'cyb_lincomb_strided_batched_f64',
              'cyb_lincomb_strided_batched_c128', 'cyb_scale_axis_batched_f64', 'cyb_mask_gather_batched_f64',
              'cyb_mask_scatter_batched_f64', 'cyb_seg_binary', 'cyb_seg_reduce', 'cyb_seg_compact', 'cyb_trace_grouped_f64',
              'cyb_outer_grouped_f64', 'cyb_tree_axis_f64', 'cyb_expm_small_batched_f64', 'cyb_dot_batched_c128',
              'cyb_gemm_grouped_enqueue_f64', 'cyb_truncate_select_f64', 'cyb_gram_schmidt_f64'}
    assert {c.entry for c in calls} == wanted
    assert all(a.entry != b.entry for a, b in zip(calls, calls[1:]))          # neighbours differ in their descriptor struct
    _check_reference_shapes(calls)
    # every call has inputs of its own: no two calls of one entry share a reference result
    for e in wanted:
        same = [c for c in calls if c.entry == e]
        firsts = [next(iter(c.expected.values())).tobytes() for c in same]
        assert len(set(firsts)) == len(same)
    # a descriptor image of the small ring stays below the first slot size (64 KiB): no slot grows, which would synchronise
    assert max(C.sizeof(t) for t in (_lib.CopyDesc, _lib.OuterRec, _lib.TreeAxisRec, _lib.TraceTerm, _lib.LincombDesc)) * 8 < 1 << 16
    # the segment reduction of the sequence has a multi-chunk segment: workspace slot 6 is first allocated in flight
    assert any(c.entry == 'cyb_seg_reduce' and c.ws_bytes[0] == 6 and c.ws_bytes[1] > 0 for c in calls)


def test_big_ring_sequence_meets_its_conditions():
    calls = cs.big_ring_sequence()
    small, big = cs.count_uploads(calls)
    assert big >= 20 and big >= 2 * K['kBig'] and small >= 20
    for c in calls:
        if c.big_uploads:
            assert c.image_bytes_min > K['kBigBytes'] and c.image_bytes_min < 2 * K['kBigBytes']   # (a big slot starts at 2 kBigBytes)
    assert all(a.big_uploads != b.big_uploads for a, b in zip(calls, calls[1:]))                    # interleaved
    _check_reference_shapes(calls)
    c = calls[0]
    assert sorted(map(tuple, c.expected['o'])) == sorted(map(tuple, c.inputs['s']))                 # a row permutation


def test_growth_sequences_exceed_the_capacity_rule():
    seqs = cs.growth_sequences()
    assert set(seqs) == {0, 2}
    for slot, s in seqs.items():
        assert all(c.ws_bytes[0] == slot for c in s['before'] + [s['grow']] + s['after'])
        left = cs.workspace_capacity(s['before'][0].ws_bytes[1])      # the first call allocates; the second must fit in it
        assert all(c.ws_bytes[1] <= left for c in s['before'] + s['after'])
        assert s['grow'].ws_bytes[1] > left
        assert sum(a.nbytes for a in list(s['grow'].inputs.values()) + list(s['grow'].outputs.values())) < 64 * cs.MIB
        assert len({c.entry for c in s['before']}) == 2               # two entries share the slot
        _check_reference_shapes(s['before'] + [s['grow']] + s['after'])
    assert cs.workspace_capacity(0) == cs.MIB
    # slot 6 cannot be outgrown below 64 MiB: 16 bytes per chunk of 16384 elements
    chunks_needed = cs.workspace_capacity(16 * 3 + 4) // 16 + 1
    assert chunks_needed * cs.SEG_CHUNK > 64 * cs.MIB                 # even with one byte per element


def test_references_agree_with_plain_numpy():
    """the references that are written as formulas over descriptors, recomputed the long way"""
    rng = np.random.default_rng(7)
    c = cs.trace_case(rng)
    for i in range(3):
        s = c.inputs[f's{i}']
        assert np.allclose(c.expected[f'o{i}'], sum(s[t, :, t] for t in range(s.shape[0])), rtol=0, atol=1e-13)
    c = cs.tree_axis_case(rng)
    for i, (o, a, n, x) in enumerate(((2, 5, 3, 33), (3, 4, 2, 17), (1, 9, 4, 21))):
        want = (c.inputs[f's{i}'].reshape(o, a, n, x) * c.inputs[f'f{i}'][None, :, None, None]).reshape(o * a * n, x)
        assert np.array_equal(c.expected[f'o{i}'], want)
    c = cs.lincomb_case(rng)
    assert np.array_equal(c.expected['o0'], np.einsum('ij->ij', 0.5 * c.inputs['s0']) - 1.25 * np.einsum('ji->ij', c.inputs['t0']))
    c = cs.mask_scatter_case(rng)
    for i in range(3):
        idx, full = c.inputs[f'i{i}'], c.expected[f'o{i}']
        assert np.array_equal(full[:, idx, :], c.inputs[f'x{i}']) and np.count_nonzero(full) == c.inputs[f'x{i}'].size
    c = cs.gram_schmidt_case(rng)
    V, w = c.inputs['V'], c.expected['w']
    assert np.abs(V @ V.T - np.eye(len(V))).max() < 1e-13 and np.abs(V @ w).max() < 1e-12 * np.linalg.norm(c.outputs['w'])
    c = cs.gram_schmidt_case(rng, n=5000, m=64, alias=True)
    v, w0 = c.inputs['V'], c.outputs['w']
    assert np.allclose(c.expected['w'], w0 - 64 * (v @ w0) * v, rtol=0, atol=1e-12 * 65 * np.linalg.norm(w0))
    c = cs.truncate_case(rng)
    s_all = np.concatenate([c.inputs[f's{i}'] for i in range(3)])
    top = np.zeros(len(s_all), dtype=np.uint8)
    top[np.argsort(-s_all, kind='stable')[:50]] = 1
    assert np.array_equal(c.expected['mask'], top)
    assert abs(c.expected['res'][0] - np.sum(s_all[top == 0] ** 2)) < 1e-13 * np.sum(s_all ** 2)
    assert list(c.expected['res'][2:].view(np.int64)) == [int(top[:40].sum()), int(top[40:100].sum()), int(top[100:].sum())]
    c = cs.seg_compact_case(rng)
    assert np.array_equal(c.expected['keep'][50:50 + c.expected['counts'][1]], np.flatnonzero(c.inputs['a1']))
    c = cs.extremum_case(rng)
    assert c.expected['r'][0] == np.abs(c.inputs['x']).max() and c.expected['r'][1:].view(np.int64)[0] == np.abs(c.inputs['x']).argmax()
    ch = cs.stream_chain()
    a, b = ch['calls'][0].inputs['a'], ch['calls'][0].inputs['b']
    assert np.allclose(ch['calls'][6].expected['f'], 3 * (a @ b).T, rtol=1e-13, atol=0)
    assert np.isclose(ch['calls'][3].expected['r'][0], (a @ b).sum(), rtol=1e-12)
    assert len(ch['first']) + len(ch['second']) + len(ch['final']) == len(ch['calls'])


def test_workspace_formulas_restate_the_sources():
    """the byte counts the growth test relies on, against the constants of the kernels' source files"""
    src = lambda f: open(os.path.join(cs.ROOT, 'cyten_amd', 'csrc', f)).read()   # noqa: E731
    kv = src('krylov_vec.hip')
    assert f'GS_MAX_M = {cs.GS_MAX_M};' in kv and f'GS_MAX_GRID = {cs.GS_MAX_GRID};' in kv
    assert 'sizeof(double) * (np + 4 * GS_MAX_M)' in kv
    tr = src('truncation.hip')
    assert re.search(r'NMAX = %d\b' % cs.TRUNC_LDS_MAX, tr) and re.search(r'NBIG = %d\b' % cs.TRUNC_MAX, tr)
    assert re.search(r'kChunk = %d\b' % cs.SEG_CHUNK, src('segment_ops.hip'))
    assert 'size_t ncap = bytes + bytes / 4 + (1 << 20);' in src('api.hip')
    assert cs.gs_ws_bytes(cs.GS_MAX_GRID * 256 - 3, 64) == 8 * (2048 * 65 * 2 + 256)
    assert cs.gs_ws_bytes(cs.GS_MAX_GRID * 256 + 257, 5) == 8 * (1025 * 6 * 2 + 256)     # two tiles per workgroup
    assert cs.truncate_ws_bytes(60000) == 480000 + 65536 * 13
