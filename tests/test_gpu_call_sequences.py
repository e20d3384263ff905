"""What one C-ABI call leaves behind for the next: descriptor ring, grow-only workspaces, stream switch, error state.

The oracle (call_sequence_cases.py): the same call with the same inputs on a QUIET context -- a second context of its own,
synchronised before and after every call -- gives the same bytes, and the quiet result is held against numpy.

Part A runs each sequence with the host ahead of the device.  A *gate* (``torch.cuda._sleep``, or a timed grouped GEMM where
this torch has none) keeps the stream busy while the calls are enqueued; it lasts twice the host time the whole sequence took
on the quiet context, at most 200 ms.  Reading the code shows where the context itself makes the host wait, and one gate in
front of a sequence cannot outlast those waits:

  * ``cyb_ctx_s::upload`` synchronises on an event at most kSlots/2 uploads old from upload kSlots on (kBig/2 and kBig in the
    ring of large images): the host can never be more than kSlots/2 uploads ahead, and a single gate is over when the 32nd
    upload of a sequence returns;
  * ``cyb_ctx_s::workspace`` synchronises the stream before it frees a slot that has to grow.

So a new gate of the same length goes in front of every stretch of kEvStride uploads (kBig/4 big ones) and behind a growing
call (``gate_points``; test_call_sequences.py shows that a gate younger than every awaited event is then always queued).  THE LEAD
CONDITION, asserted and not measured: when a call returns, the youngest gate has not finished -- at the last call of every
sequence, and at every other call except a growing one.  A sequence that fails it fails the test.

No entry of the sequences waits inside: none was moved out.  The decompositions (``matrix_amax`` reads the block maxima back)
wait by design and appear in part B only.  Times printed here (``-s``) are for the record; nothing but the lead depends on time.
"""
import contextlib
import ctypes as C
import functools
import time

import numpy as np
import pytest

import call_sequence_cases as cs
from cyten_amd import _lib

pytestmark = pytest.mark.gpu
K = cs.ring_constants()
GATE_CAP_MS = 200.0
DECOMP_TOL = 1e-10


# ---------------------------------------------------------------------------------------------------------------- plumbing

def fresh_backend():
    """a HipBlockBackend on a context of its own (the public constructor shares one context per device)"""
    import torch
    assert torch.cuda.is_available(), 'GPU tests selected but no HIP device is visible'
    from cyten_amd.block_backend import HipBlockBackend
    from cyten_amd.runtime import Context
    b = HipBlockBackend('cuda:0')
    b.ctx = Context(0)      # (in place of the shared one the constructor looked up)
    b.lib = b.ctx.lib
    return b


@contextlib.contextmanager
def backends(n=1):
    import torch
    made = [fresh_backend() for _ in range(n)]
    try:
        yield made
    finally:
        torch.cuda.synchronize()
        for b in made:
            b.lib.cyb_ctx_destroy(b.ctx.handle)


def _alloc(calls, shared=False):
    """device buffers of every call (one namespace per call, or one for a dependent chain), uploaded and synchronised"""
    import torch
    spaces, common = [], {}
    for c in calls:
        ns = common if shared else {}
        for name, arr in list(c.inputs.items()) + list(c.outputs.items()):
            if name not in ns:
                a = np.ascontiguousarray(arr)
                ns[name] = (torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to('cuda:0'), a.dtype, a.shape)
        spaces.append(ns)
    torch.cuda.synchronize()
    return spaces


def _ptrs(ns):
    return {k: t.data_ptr() for k, (t, _, _) in ns.items()}


def _download(calls, spaces):
    out = []
    for c, ns in zip(calls, spaces):
        out.append({name: ns[name][0].cpu().numpy().view(ns[name][1]).reshape(ns[name][2]) for name in c.outputs})
    return out


def _err(b):
    return b.lib.cyb_last_error().decode(errors='replace')


def run_quiet(calls, shared=False):
    """every call alone on a context of its own, checked against numpy; returns the outputs and the host time of the calls"""
    with backends() as (q,):
        spaces = _alloc(calls, shared)
        host = 0.0
        for c, ns in zip(calls, spaces):
            p = _ptrs(ns)
            q.synchronize()
            t0 = time.perf_counter()
            st = c.launch(q.lib, q.ctx.handle, p)
            host += time.perf_counter() - t0
            q.synchronize()
            assert st == _lib.CYB_OK, (c.entry, st, _err(q))
        got = _download(calls, spaces)
    for c, g in zip(calls, got):
        c.check(g)
    return got, host


def same_bytes(calls, got, want, what):
    for i, (c, g, w) in enumerate(zip(calls, got, want)):
        for name in c.outputs:
            assert g[name].tobytes() == w[name].tobytes(), (
                f'{what}: call {i} ({c.entry}), output {name!r}: {int((g[name].view(np.uint8) != w[name].view(np.uint8)).sum())} '
                'bytes differ from the quiet context')


class Gate:
    """keeps the current stream busy for a given time"""

    def __init__(self):
        import torch
        self.torch = torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if hasattr(torch.cuda, '_sleep'):
            cycles = 4_000_000
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            self.cycles_per_ms = cycles / e0.elapsed_time(e1)
            self.block = None
        else:   # one large grouped-GEMM problem on a context of its own, timed once
            self.block = fresh_backend()
            n = 4096
            self.ops = [torch.ones(n * n, dtype=torch.float64, device='cuda:0') for _ in range(3)]
            self.prob = (_lib.GemmProb * 1)(_lib.GemmProb(self.ops[2].data_ptr(), n, n, n, 0, 1, 1.0, 0.0))
            self.seg = (_lib.GemmSeg * 1)(_lib.GemmSeg(self.ops[0].data_ptr(), self.ops[1].data_ptr(), n, n, 1, n, 1))
            self._gemm()
            torch.cuda.synchronize()
            e0.record()
            self._gemm()
            e1.record()
            e1.synchronize()
            self.gemm_ms = e0.elapsed_time(e1)

    def _gemm(self):
        self.block.ctx.sync_stream()
        _lib.check(self.block.lib.cyb_gemm_grouped_enqueue_f64(self.block.ctx.handle, self.prob, 1, self.seg, 1))

    def enqueue(self, ms):
        """returns the event that ends the gate"""
        if self.block is None:
            self.torch.cuda._sleep(int(self.cycles_per_ms * ms))
        else:
            for _ in range(max(1, int(np.ceil(ms / self.gemm_ms)))):
                self._gemm()
        end = self.torch.cuda.Event()
        end.record()
        return end


@functools.lru_cache(maxsize=None)
def gate():
    return Gate()


@pytest.fixture(scope='module', autouse=True)
def _release_gate():
    yield
    if gate.cache_info().currsize:
        g = gate()
        gate.cache_clear()
        if g.block is not None:     # the context of the GEMM fallback
            g.torch.cuda.synchronize()
            g.block.lib.cyb_ctx_destroy(g.block.ctx.handle)


def gate_ms_for(host_seconds):
    return min(GATE_CAP_MS, 2e3 * host_seconds)


def run_gated(b, calls, spaces, gate_ms, gate_at, waits=(), what=''):
    """Enqueue `calls` on context `b` with no host wait of our own, a gate in front of every call listed in `gate_at`;
    asserts the lead condition, then synchronises once.  Returns the host time of the loop."""
    import torch
    g = gate()
    b.ctx.sync_stream()
    ptrs = [_ptrs(ns) for ns in spaces]
    gate_at = set(gate_at)
    torch.cuda.synchronize()
    status, behind = [], []
    t0 = time.perf_counter()
    for i, (c, p) in enumerate(zip(calls, ptrs)):
        if i in gate_at:
            end = g.enqueue(gate_ms)
        status.append(c.launch(b.lib, b.ctx.handle, p))
        behind.append(not end.query())
    host = time.perf_counter() - t0
    done = torch.cuda.Event()
    done.record()
    done.synchronize()
    for i, (c, st) in enumerate(zip(calls, status)):
        assert st == _lib.CYB_OK, (what, i, c.entry, st, _err(b))
    lost = [i for i, ok in enumerate(behind) if not ok and i not in waits]
    assert behind[-1] and not lost, (
        f'{what}: the lead was not held -- the youngest gate ({gate_ms:.2f} ms) had finished when call(s) {lost or [len(calls) - 1]} '
        f'({[calls[i].entry for i in (lost or [len(calls) - 1])]}) returned: an entry waits for the device inside')
    return host


def report(what, calls, quiet_host, gate_ms, n_gates, host):
    small, big = cs.count_uploads(calls)
    print(f'\n[call-sequences] {what}: {len(calls)} calls, {small} small-ring + {big} big-ring uploads, quiet enqueue '
          f'{1e3 * quiet_host:.2f} ms, gate {gate_ms:.2f} ms x {n_gates}, gated enqueue {1e3 * host:.2f} ms, lead held')


# ---------------------------------------------------------------------------------------------------------------- part A

@functools.lru_cache(maxsize=None)
def small_ring():
    calls = cs.small_ring_sequence()
    got, host = run_quiet(calls)
    return calls, got, host


@pytest.mark.parametrize('phase', [0, 5, 13])
def test_small_ring_refilled_behind_the_gate(phase):
    """A1: 95 calls of 19 entries (90 uploads, each slot refilled at least twice) from three ring phases.

    What this can and cannot see: because upload() itself holds the host back, the device is never more than kSlots/2 = 16
    uploads behind the host here or in any other test.  Every call of the sequence launches its consumer right after its one
    upload, so the run shows that slots are not recycled too EARLY by upload()'s own arithmetic and that the entries do not
    mix up each other's images; a call that launched a consumer more than kSlots/2 - 1 uploads after filling its slot would
    break the rule without a wrong byte here -- that distance is pinned by the model in test_call_sequences.py alone."""
    calls, want, quiet_host = small_ring()
    with backends() as (b,):
        for d in cs.dummy_upload_calls(phase):
            (ns,) = _alloc([d])
            assert d.launch(b.lib, b.ctx.handle, _ptrs(ns)) == _lib.CYB_OK
        b.synchronize()
        spaces = _alloc(calls)
        pts = cs.gate_points(calls, K)
        ms = gate_ms_for(quiet_host)
        host = run_gated(b, calls, spaces, ms, pts, what=f'small ring, phase {phase}')
        got = _download(calls, spaces)
    same_bytes(calls, got, want, f'small ring, phase {phase}')
    report(f'A1 small ring, phase {phase}', calls, quiet_host, ms, len(pts), host)


def test_big_ring_refilled_behind_the_gate():
    """A2: 20 descriptor images above kBigBytes (607 tiny copies each), a small-ring call after each"""
    calls = cs.big_ring_sequence()
    want, quiet_host = run_quiet(calls)
    with backends() as (b,):
        spaces = _alloc(calls)
        pts = cs.gate_points(calls, K)
        ms = gate_ms_for(quiet_host)
        host = run_gated(b, calls, spaces, ms, pts, what='big ring')
        got = _download(calls, spaces)
    same_bytes(calls, got, want, 'big ring')
    report('A2 big ring', calls, quiet_host, ms, len(pts), host)


@pytest.mark.parametrize('slot', [0, 2])
def test_workspace_growth_in_flight(slot):
    """A3: small calls of two entries on one slot, a call that outgrows what they left, the small calls again -- on a context
    made here, so the slot starts empty.  The growing call synchronises the stream by design (its lead is not asserted); a
    gate behind it puts the host ahead again for the calls that find the new, uninitialised memory.  Slot 6 is left out:
    see growth_sequences()."""
    s = cs.growth_sequences()[slot]
    calls = s['before'] + [s['grow']] + s['after']
    grow_at = len(s['before'])
    want, quiet_host = run_quiet(calls)
    with backends() as (b,):
        spaces = _alloc(calls)
        ms = gate_ms_for(quiet_host)
        host = run_gated(b, calls, spaces, ms, [0, grow_at, grow_at + 1], waits=(grow_at,), what=f'growth of slot {slot}')
        got = _download(calls, spaces)
    same_bytes(calls, got, want, f'growth of slot {slot}')
    report(f'A3 growth of slot {slot}', calls, quiet_host, ms, 3, host)


def test_stream_switch_in_a_dependent_chain():
    """A4: GEMM -> copy -> dot on the first stream behind one gate; reduce, axpby and dot on a second stream
    (``torch.cuda.stream`` + ``sync_stream``), reading the first half's outputs and reusing ring and workspace slots 0 and 6;
    a final call back on the first stream.  One host wait, at the end."""
    import torch
    ch = cs.stream_chain()
    calls = ch['calls']
    want, quiet_host = run_quiet(calls, shared=True)
    with backends() as (b,):
        spaces = _alloc(calls, shared=True)
        p = _ptrs(spaces[0])
        s2 = torch.cuda.Stream()
        with torch.cuda.stream(s2):      # (the runtime sets a stream's hardware queue up on its first use: not part of the chain)
            torch.zeros(8, device='cuda:0')
        ms = gate_ms_for(quiet_host)
        b.ctx.sync_stream()
        torch.cuda.synchronize()
        status, behind = [], []

        def run(part):
            for c in part:
                status.append(c.launch(b.lib, b.ctx.handle, p))
                behind.append(not end.query())
        t0 = time.perf_counter()
        end = gate().enqueue(ms)
        run(ch['first'])
        with torch.cuda.stream(s2):
            b.ctx.sync_stream()
            run(ch['second'])
        b.ctx.sync_stream()
        run(ch['final'])
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        assert status == [_lib.CYB_OK] * len(calls), (status, _err(b))
        assert all(behind), (f'stream switch: the lead was not held -- the gate ({ms:.2f} ms) had finished when call '
                             f'{behind.index(False)} ({calls[behind.index(False)].entry}) returned, {1e3 * host:.2f} ms into the chain')
        got = _download(calls, spaces)
    for c, g in zip(calls, got):
        c.check(g)
    same_bytes(calls, got, want, 'stream switch')
    report('A4 stream switch', calls, quiet_host, ms, 1, host)


# ---------------------------------------------------------------------------------------------------------------- part B

def run_plain(b, calls):
    """the calls back to back on context `b`, one wait at the end"""
    spaces = _alloc(calls)
    b.ctx.sync_stream()
    for c, ns in zip(calls, spaces):
        st = c.launch(b.lib, b.ctx.handle, _ptrs(ns))
        assert st == _lib.CYB_OK, (c.entry, st, _err(b))
    b.synchronize()
    return _download(calls, spaces)


def _rng(*k):
    return np.random.default_rng([41, *k])


FAILING = [   # (id, failing call, status, fragment of its message, healthy call of the same entry, healthy call of another entry on the slot)
    ('invalid-truncate', lambda: cs.truncate_case(_rng(0), chi_min=0), _lib.CYB_ERR_INVALID, 'chi_min',
     lambda: cs.truncate_case(_rng(1)), lambda: cs.extremum_case(_rng(2))),
    ('unsupported-truncate', lambda: cs.truncate_case(_rng(3), sizes=(cs.TRUNC_MAX + 1,), chi_max=10), _lib.CYB_ERR_UNSUPPORTED, '65537 values',
     lambda: cs.truncate_case(_rng(4)), lambda: cs.extremum_case(_rng(5))),
    ('unsupported-gram-schmidt', lambda: cs.gram_schmidt_case(_rng(6), n=64, m=cs.GS_MAX_M + 1, alias=True), _lib.CYB_ERR_UNSUPPORTED,
     '65 basis vectors', lambda: cs.gram_schmidt_case(_rng(7)), lambda: cs.dot_c128_case(_rng(8))),
]


@pytest.mark.parametrize('case', FAILING, ids=[f[0] for f in FAILING])
def test_state_after_a_rejected_call(case):
    """CYB_ERR_INVALID (a case of test_gpu_cabi_errors.py) and CYB_ERR_UNSUPPORTED: the call writes nothing, the next healthy
    calls of the same entry and of another entry on the same workspace slot give the quiet context's bytes, and
    cyb_last_error() names this failure, not the one before it"""
    _, bad, status, fragment, same, other = case
    bad, healthy = bad(), [same(), other()]
    want, _ = run_quiet(healthy)
    with backends() as (b,):
        assert b.lib.cyb_copy_strided_batched(b.ctx.handle, None, 1, 3) == _lib.CYB_ERR_INVALID     # an older failure
        assert 'cyb_copy_strided_batched' in _err(b)
        run_plain(b, [same()])                                                                       # the slot is in use
        (ns,) = _alloc([bad])
        assert bad.launch(b.lib, b.ctx.handle, _ptrs(ns)) == status
        msg = _err(b)
        assert fragment in msg and bad.entry in msg and 'cyb_copy_strided_batched' not in msg, msg
        b.synchronize()
        bad.check(_download([bad], [ns])[0])                                                         # outputs untouched
        got = run_plain(b, healthy)
        assert _err(b) == msg                                                                        # healthy calls leave it alone
    same_bytes(healthy, got, want, 'after ' + case[0])


def _svd_ok(a, U, S, Vh, tol=DECOMP_TOL):
    """the acceptance criteria of helpers.check_svd_invariants, for real and complex blocks (test_gpu_special_values.py)"""
    k = min(a.shape)
    nrm = np.linalg.norm(a)
    assert np.all(S >= 0) and np.all(S[:-1] >= S[1:] - tol * nrm)
    assert np.abs(S - np.linalg.svd(a, compute_uv=False)).max() <= tol * nrm
    assert np.abs((U * S) @ Vh - a).max() <= tol * nrm
    assert np.abs(U.conj().T @ U - np.eye(k)).max() <= tol and np.abs(Vh @ Vh.conj().T - np.eye(k)).max() <= tol


def _eigh_ok(h, w, v, tol=DECOMP_TOL):
    nrm = np.linalg.norm(h)
    assert np.abs(np.sort(w) - np.linalg.eigvalsh(h)).max() <= tol * nrm
    assert np.abs(h @ v - v * w).max() <= tol * nrm
    assert np.abs(v.conj().T @ v - np.eye(len(w))).max() <= tol


def _decomp_call(b, kind, cplx, mats):
    """one cyb_{svd,eigh}_batched_{f64,c128} call with an info array; returns status, info, per-block factors (numpy)"""
    import torch
    dt = np.complex128 if cplx else np.float64

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=a.dtype)).to('cuda:0')
    A = [dev(a.astype(dt)) for a in mats]
    outs, descs = [], []
    for a, t in zip(mats, A):
        m, n = a.shape
        k = min(m, n)
        if kind == 'svd':
            o = [dev(np.full((m, k), cs.SENTINEL, dtype=dt)), dev(np.full(k, cs.SENTINEL)), dev(np.full((k, n), cs.SENTINEL, dtype=dt))]
            descs.append(_lib.SvdDesc(t.data_ptr(), n, m, n, o[0].data_ptr(), k, o[1].data_ptr(), o[2].data_ptr(), n))
        else:
            o = [dev(np.full(n, cs.SENTINEL)), dev(np.full((n, n), cs.SENTINEL, dtype=dt))]
            descs.append(_lib.EighDesc(t.data_ptr(), n, n, o[0].data_ptr(), o[1].data_ptr(), n))
        outs.append(o)
    torch.cuda.synchronize()
    info = (C.c_int32 * len(mats))(*([7] * len(mats)))
    fn = getattr(b.lib, f'cyb_{kind}_batched_{"c128" if cplx else "f64"}')
    arr = ((_lib.SvdDesc if kind == 'svd' else _lib.EighDesc) * len(mats))(*descs)
    b.ctx.sync_stream()
    st = fn(b.ctx.handle, arr, len(mats), info)
    b.synchronize()
    return st, list(info), [[x.cpu().numpy() for x in o] for o in outs]


def _decomp_blocks(kind, cplx, seed):
    rng = np.random.default_rng([43, seed])

    def block(shape):
        a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
        return (a + a.conj().T) / 2 if kind == 'eigh' else a
    if kind == 'svd':     # the complex list mixes the in-LDS route (the middle block) with the device-memory route
        shapes = [(100, 70), (20, 20), (130, 100)] if cplx else [(33, 17), (20, 20), (64, 40)]
    else:
        shapes = [(100, 100), (33, 33), (70, 70)] if cplx else [(33, 33), (20, 20), (40, 40)]
    return [block(s) for s in shapes]


@pytest.mark.parametrize('bad_at', [1, 0])
@pytest.mark.parametrize('kind,cplx', [('svd', False), ('eigh', False), ('svd', True), ('eigh', True)],
                         ids=['svd_f64', 'eigh_f64', 'svd_c128', 'eigh_c128'])
def test_state_after_a_list_with_a_nan_block(kind, cplx, bad_at):
    """CYB_ERR_NOCONV: a list of three blocks with one NaN block.  info is -1 for that block and a sweep count (>= 0) for the
    others (include/cyten_amd.h), whose factors pass the SVD / eigh invariants at 1e-10 -- test_nonfinite_* checks the raise
    and a LATER healthy call at the backend level, not the healthy blocks of the failed list itself.  Then the state: the
    next healthy list of the same entry decomposes (compared with numpy only: the Jacobi routes do not document run-to-run
    identity), calls of other entries on workspace slots 0 and 2 give the quiet context's bytes, the message is this call's."""
    mats = _decomp_blocks(kind, cplx, 0)
    poisoned = [m.copy() for m in mats]
    if kind == 'eigh':
        poisoned[bad_at][2, 1] = poisoned[bad_at][1, 2] = np.nan
    else:
        poisoned[bad_at][2, 1] = np.nan
    others = [cs.dot_c128_case(_rng(9)), cs.extremum_case(_rng(10)), cs.truncate_case(_rng(11))]
    want, _ = run_quiet(others)
    ok = _svd_ok if kind == 'svd' else _eigh_ok
    with backends() as (b,):
        assert b.lib.cyb_copy_strided_batched(b.ctx.handle, None, 1, 3) == _lib.CYB_ERR_INVALID     # an older failure
        st, info, outs = _decomp_call(b, kind, cplx, poisoned)
        msg = _err(b)
        assert st == _lib.CYB_ERR_NOCONV, (st, msg)
        assert 'cyb_copy_strided_batched' not in msg and msg
        assert info[bad_at] == -1 and all(info[i] >= 0 for i in range(3) if i != bad_at), info
        for i in range(3):
            if i != bad_at:
                ok(mats[i], *outs[i])
        got = run_plain(b, others)
        st, info, outs = _decomp_call(b, kind, cplx, mats)
        assert st == _lib.CYB_OK and all(i >= 0 for i in info), (st, info, _err(b))
        for a, o in zip(mats, outs):
            ok(a, *o)
        assert _err(b) == msg
    same_bytes(others, got, want, f'after a NaN block in {kind}')


def test_wait_free_calls_around_a_decomposition_that_waits():
    """five wait-free calls, a real SVD (which reads the block maxima back before it starts), five more: one wait of our own
    at the end, all ten equal to the quiet context"""
    builders = [cs.seg_reduce_case, cs.dot_c128_case, cs.truncate_case, cs.gemm_case, cs.gram_schmidt_case,
                cs.extremum_case, cs.lincomb_case, cs.seg_compact_case, cs.dot_c128_case, cs.trace_case]
    calls = [f(_rng(20, i)) for i, f in enumerate(builders)]
    want, _ = run_quiet(calls)
    a = _rng(21).standard_normal((100, 100))
    with backends() as (b,):
        spaces = _alloc(calls)
        A = b.as_block(a)
        b.synchronize()
        for c, ns in zip(calls[:5], spaces[:5]):
            assert c.launch(b.lib, b.ctx.handle, _ptrs(ns)) == _lib.CYB_OK
        (U, S, Vh), = b.matrix_svd_batched([A])
        for c, ns in zip(calls[5:], spaces[5:]):
            assert c.launch(b.lib, b.ctx.handle, _ptrs(ns)) == _lib.CYB_OK
        b.synchronize()
        got = _download(calls, spaces)
        _svd_ok(a, b.to_numpy(U), b.to_numpy(S), b.to_numpy(Vh))
    same_bytes(calls, got, want, 'around an SVD')


# ---------------------------------------------------------------------------------------------------------------- part C

def test_deferred_backend_after_a_permanent_failure():
    """One batch: the SVD of a NaN block, two healthy SVDs with the same option, an unrelated product.  Only forcing the bad
    block's outputs raises; the healthy blocks and the product materialise; a later flush() for new work neither raises nor
    runs the bad block again; the bad node has left the queue."""
    from cyten_amd.deferred import DeferredBlockBackend
    rng = _rng(30)
    dbb = DeferredBlockBackend('cuda:0')
    good = [rng.standard_normal((24, 20)), rng.standard_normal((20, 31))]
    bad = rng.standard_normal((22, 22))
    bad[3, 4] = np.nan
    a, c = rng.standard_normal((17, 9)), rng.standard_normal((9, 13))
    u0, s0, v0 = dbb.matrix_svd(dbb.as_block(good[0]))
    bad_block = dbb.as_block(bad)
    ub, sb, vb = dbb.matrix_svd(bad_block)
    u1, s1, v1 = dbb.matrix_svd(dbb.as_block(good[1]))
    prod = dbb.matrix_dot(dbb.as_block(a), dbb.as_block(c))
    # work behind the bad block in the same batch: product -> decomposition -> product (tdot -> qr -> tdot)
    e = dbb.as_block(rng.standard_normal((22, 22)))
    dep1 = dbb.matrix_dot(ub, e)
    dq, dr = dbb.matrix_qr(dep1, False)
    dep2 = dbb.matrix_dot(dq, e)

    def bad_node_queued():
        return any(n.block is bad_block for n in dbb._pending_decomp)
    _svd_ok(good[0], dbb.to_numpy(u0), dbb.to_numpy(s0), dbb.to_numpy(v0))       # the first observation flushes: it does not raise
    _svd_ok(good[1], dbb.to_numpy(u1), dbb.to_numpy(s1), dbb.to_numpy(v1))
    np.testing.assert_allclose(dbb.to_numpy(prod), a @ c, rtol=0, atol=1e-12)
    assert not bad_node_queued()
    with pytest.raises(_lib.LinAlgError):
        dbb.to_numpy(sb)
    assert not bad_node_queued()
    # new work: flush() neither raises nor runs the bad block or anything behind it
    batches, launches = dbb.n_decomp_batches, dbb.n_flushes
    x = rng.standard_normal((15, 15))
    w, v = dbb.eigh(dbb.as_block(x + x.T))
    later = dbb.matrix_dot(dbb.as_block(a), dbb.as_block(c))
    dbb.flush()
    assert dbb.n_decomp_batches == batches + 1 and dbb.n_flushes == launches + 1 and not bad_node_queued()
    _eigh_ok(x + x.T, dbb.to_numpy(w), dbb.to_numpy(v))
    np.testing.assert_allclose(dbb.to_numpy(later), a @ c, rtol=0, atol=1e-12)
    dbb.synchronize()
    dbb.flush()                                                                   # ... and again, with nothing new
    assert dbb.n_decomp_batches == batches + 1 and dbb.n_flushes == launches + 1
    with pytest.raises(_lib.LinAlgError):                                         # still only its own outputs raise
        dbb.to_numpy(ub)
    for dependent in (dep1, dq, dr, dep2):                                        # what depends on them says so, and is not run
        with pytest.raises(RuntimeError, match='decomposition that failed'):
            dbb.to_numpy(dependent)
    assert dbb.n_decomp_batches == batches + 1 and dbb.n_flushes == launches + 1 and not bad_node_queued()
