"""Which C-ABI entry every block of a decomposition call reaches (cyten_amd/decomp.py): the embedded float64 route above the
`COMPLEX_*_EMBED_MIN` thresholds, the complex kernels below them and for what the embedded route hands back, the direct
entries, and the three forms of the real SVD.  The shapes are the smallest on either side of each threshold.

The routes are observed, not inferred: `bb.lib` is replaced by a forwarding proxy that notes the name and the item count of
every `cyb_*` call and changes nothing else."""
import numpy as np
import pytest

from test_gpu_complex import _copied_column_blocks, _cqr_check, _csvd_check, crandn

pytestmark = pytest.mark.gpu


class RecordingLib:
    """Forwards every attribute to the loaded library; calls of `cyb_*` entries are appended to `log` as (name, n), n being
    the item count (the third argument of every batched entry) or None for entries without one."""

    def __init__(self, lib):
        self._lib = lib
        self.log = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('cyb_') or not callable(fn):
            return fn

        def call(*args):
            n = args[2] if len(args) > 2 and isinstance(args[2], (int, np.integer)) else None
            self.log.append((name, None if n is None else int(n)))
            return fn(*args)
        return call

    def calls(self, prefix):
        return [c for c in self.log if c[0].startswith(prefix)]


@pytest.fixture
def rec(bb, monkeypatch):
    proxy = RecordingLib(bb.lib)
    monkeypatch.setattr(bb, 'lib', proxy)
    return proxy


def _blocks(bb, mats):
    return [bb.as_block(m) for m in mats]


def _hermitian(rng, n):
    z = crandn(rng, (n, n))
    return z + z.conj().T


def test_complex_svd_routes(bb, rng, rec):
    mats = [crandn(rng, s) for s in [(96, 96), (95, 95), (12, 7)]]
    res = bb.matrix_svd_batched(_blocks(bb, mats))
    assert rec.calls('cyb_svd_') == [('cyb_svd_batched_ex_f64', 1), ('cyb_svd_batched_c128', 2)]
    for m, (u, s, vh) in zip(mats, res):
        _csvd_check(m, bb.to_numpy(u), bb.to_numpy(s), bb.to_numpy(vh))
    del rec.log[:]
    direct = bb.matrix_svd_batched_complex_direct(bb.contiguous_many(_blocks(bb, mats)))
    assert rec.calls('cyb_svd_') == [('cyb_svd_batched_c128', 3)]
    for m, (u, s, vh) in zip(mats, direct):
        _csvd_check(m, bb.to_numpy(u), bb.to_numpy(s), bb.to_numpy(vh))
    # the direct entry leaves the threshold alone: the class constant, no instance attribute
    assert bb.COMPLEX_SVD_EMBED_MIN == 96
    assert 'COMPLEX_SVD_EMBED_MIN' not in vars(bb)


def test_real_svd_entries(bb, rng, rec):
    mats = [rng.standard_normal(s) for s in [(40, 30), (5, 5)]]
    res = bb.matrix_svd_batched(_blocks(bb, mats))
    assert rec.calls('cyb_svd_') == [('cyb_svd_batched_f64', 2)]
    for m, (u, s, vh) in zip(mats, res):
        u, s, vh = bb.to_numpy(u), bb.to_numpy(s), bb.to_numpy(vh)
        assert np.abs((u * s) @ vh - m).max() <= 1e-10 * np.linalg.norm(m)
        assert np.abs(s - np.linalg.svd(m, compute_uv=False)).max() <= 1e-10 * np.linalg.norm(m)
    del rec.log[:]
    res, ranks = bb.matrix_svd_batched(_blocks(bb, mats), null_vectors=False, return_rank=True)
    assert rec.calls('cyb_svd_') == [('cyb_svd_batched_ex_f64', 2)]
    assert ranks == [30, 5]
    for m, (u, s, vh) in zip(mats, res):
        assert np.abs(bb.to_numpy(s) - np.linalg.svd(m, compute_uv=False)).max() <= 1e-10 * np.linalg.norm(m)
    outs = [(bb.zeros((40, 30)), bb.zeros((30,)), bb.zeros((30, 30))), (bb.zeros((5, 5)), bb.zeros((5,)), bb.zeros((5, 4)))]
    with pytest.raises(ValueError, match=r'matrix_svd_batched: outs\[i\] must be contiguous \(m,k\), \(k,\), \(k,n\) blocks'):
        bb.matrix_svd_batched(_blocks(bb, mats), outs=outs)


@pytest.mark.parametrize('full', [False, True])
def test_complex_qr_routes(bb, rng, rec, full):
    mats = [crandn(rng, s) for s in [(48, 48), (47, 47), (10, 129), (0, 5)]]
    res = bb.matrix_qr_batched(_blocks(bb, mats), full)
    # (48, 48) and (10, 129): one real QR of their 96 x 96 and 20 x 258 embeddings; the other two: complex Householder
    assert rec.calls('cyb_qr_') == [('cyb_qr_batched_f64', 2), ('cyb_qr_batched_c128', 2)]
    for a, (q, r) in zip(mats[:3], res):
        _cqr_check(a, bb.to_numpy(q), bb.to_numpy(r), full)
    q, r = res[3]
    assert q.shape == (0, 0) and r.shape == (0, 5) and q.is_complex and r.is_complex


def test_complex_qr_falls_back_per_block(bb, rng, rec):
    """A rank-50 (150, 150) block with copied columns enters the embedded route, fails its checks there and is the only
    block of the list that the complex Householder kernels factor; the full-rank block beside it stays embedded."""
    mats = [_copied_column_blocks(rng, [(150, 150)])[0], crandn(rng, (150, 150))]
    res = bb.matrix_qr_batched(_blocks(bb, mats), False)
    qr_calls = rec.calls('cyb_qr_')
    assert qr_calls[0] == ('cyb_qr_batched_f64', 2)
    assert qr_calls[-1] == ('cyb_qr_batched_c128', 1) and [c[0] for c in qr_calls].count('cyb_qr_batched_c128') == 1
    for a, (q, r) in zip(mats, res):
        _cqr_check(a, bb.to_numpy(q), bb.to_numpy(r), False)


def test_complex_eigh_routes(bb, rng, rec):
    mats = [_hermitian(rng, n) for n in (96, 95, 9)]
    res = bb.eigh_batched(_blocks(bb, mats))
    assert rec.calls('cyb_eigh_') == [('cyb_eigh_batched_ex_f64', 1), ('cyb_eigh_batched_c128', 2)]
    for h, (w, v) in zip(mats, res):
        w, v = bb.to_numpy(w), bb.to_numpy(v)
        nrm = np.abs(h).max() * h.shape[0]
        assert np.all(np.diff(w) >= 0) and np.abs(w - np.linalg.eigvalsh(h)).max() <= 1e-10 * nrm
        assert np.abs(h @ v - v * w).max() <= 1e-10 * nrm
        assert np.abs(v.conj().T @ v - np.eye(h.shape[0])).max() <= 1e-10
    for h, (w, v) in zip(mats, bb.eigh_batched(_blocks(bb, mats), sort='>')):
        w, v = bb.to_numpy(w), bb.to_numpy(v)
        assert np.all(np.diff(w) <= 0) and np.abs(h @ v - v * w).max() <= 1e-10 * np.abs(h).max() * h.shape[0]
    for h in mats[:1] + mats[2:]:
        w = bb.eigvalsh(bb.as_block(h))
        assert w.shape == (h.shape[0],) and not w.is_complex
        assert np.abs(bb.to_numpy(w) - np.linalg.eigvalsh(h)).max() <= 1e-10 * np.abs(h).max() * h.shape[0]
    for w, v in bb.eigh_batched(_blocks(bb, mats), vectors=False):
        assert v is None
    del rec.log[:]
    direct = bb.eigh_batched_direct(bb.contiguous_many(_blocks(bb, mats)))
    assert rec.calls('cyb_eigh_') == [('cyb_eigh_batched_c128', 3)]
    for h, (w, v) in zip(mats, direct):
        assert np.abs(bb.to_numpy(w) - np.linalg.eigvalsh(h)).max() <= 1e-10 * np.abs(h).max() * h.shape[0]
    assert bb.COMPLEX_EIGH_EMBED_MIN == 96 and 'COMPLEX_EIGH_EMBED_MIN' not in vars(bb)


def test_mixed_real_and_complex_lists(bb, rng, rec):
    """One float64 and one complex block per call: the float64 block is promoted and both go to the complex kernels."""
    a, c = rng.standard_normal((20, 20)), crandn(rng, (20, 20))
    (ur, sr, vr), (uc, sc, vc) = bb.matrix_svd_batched(_blocks(bb, [a, c]))
    assert rec.calls('cyb_svd_') == [('cyb_svd_batched_c128', 2)]
    _csvd_check(a.astype(complex), bb.to_numpy(ur), bb.to_numpy(sr), bb.to_numpy(vr))
    _csvd_check(c, bb.to_numpy(uc), bb.to_numpy(sc), bb.to_numpy(vc))
    for full in (False, True):
        del rec.log[:]
        (qr_, rr), (qc, rc) = bb.matrix_qr_batched(_blocks(bb, [a, c]), full)
        assert rec.calls('cyb_qr_') == [('cyb_qr_batched_c128', 2)]
        _cqr_check(a.astype(complex), bb.to_numpy(qr_), bb.to_numpy(rr), full)
        _cqr_check(c, bb.to_numpy(qc), bb.to_numpy(rc), full)
    hs = [a + a.T, c + c.conj().T]
    del rec.log[:]
    res = bb.eigh_batched(_blocks(bb, hs))
    assert rec.calls('cyb_eigh_') == [('cyb_eigh_batched_c128', 2)]
    for h, (w, v) in zip(hs, res):
        w, v = bb.to_numpy(w), bb.to_numpy(v)
        assert w.dtype == np.float64 and v.dtype == np.complex128
        assert np.abs(w - np.linalg.eigvalsh(h)).max() <= 1e-10 * np.abs(h).max() * 20
        assert np.abs(h @ v - v * w).max() <= 1e-10 * np.abs(h).max() * 20


def test_complex_lq(bb, rng, rec):
    a = crandn(rng, (130, 60))
    (l, q), = bb.matrix_lq_batched([bb.as_block(a)])
    assert rec.calls('cyb_qr_') == [('cyb_qr_batched_f64', 1)]           # the (60, 130) transpose: embedded route
    l, q = bb.to_numpy(l), bb.to_numpy(q)
    assert l.shape == (130, 60) and q.shape == (60, 60)
    assert np.abs(l @ q - a).max() <= 1e-10 * np.linalg.norm(a) and np.abs(q @ q.conj().T - np.eye(q.shape[0])).max() <= 1e-10
    assert np.abs(np.triu(l, 1)).max() == 0.0
