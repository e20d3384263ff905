"""Direct sums on the device: one Lanczos step and one GMRES step on a two-component direct sum on pools
(krylov._FlatDirectSumOps: every vector operation one launch over the whole range) against the same step on tensors
(krylov._DirectSumOps: per-component launches), and sparse.gram_schmidt of 8 direct sums -- ONE cyb_orthonormalize_f64 call and
one download -- against the host-synchronous loop on tensors, alternating in one process.

    python scripts/direct_sum_bench.py [chi ...]        (default 1024 4096; D = 5, two config_heff operators)

Host clock around a step that ends in a device synchronise, medians of 7 after a warm-up.  Prints one line per figure."""
import statistics
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
from cyten_amd.block_backend import HipBlockBackend  # noqa: E402
from cyten_amd import direct_sum as ds, krylov, sparse, workloads as wl  # noqa: E402
from cyten_amd.direct_sum import DirectSum  # noqa: E402
from helpers import to_device_tensor  # noqa: E402


def median_ms(bb, fn, reps=7):
    fn()
    bb.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        bb.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def lanczos_step(V, w, prev, beta):
    """one step of LanczosGroundState._build_krylov without reorthogonalisation"""
    w = V.scale(1.0 / beta, w)
    x = V.matvec(w)
    alpha = float(abs(V.inner(x, w)))
    x = V.lincomb(1.0, x, -alpha, w)
    x = V.lincomb(1.0, x, -beta, prev)
    return x, V.norm(x)


def main():
    bb = HipBlockBackend('cuda:0')
    chis = [int(x) for x in sys.argv[1:]] or [1024, 4096]
    for chi in chis:
        ops, thetas = [], []
        for seed in (11, 12):
            cfg = wl.config_heff(chi, 5, seed=seed)
            dev = {k: to_device_tensor(bb, v) for k, v in cfg.items()}
            ops.append(krylov.HEffective(bb, dev['LP'], dev['W1'], dev['W2'], dev['RP']))
            thetas.append(dev['theta'])
        H = sparse.DirectSumLinearOperator(ops, bb)
        psi = DirectSum(thetas)
        t_mv = median_ms(bb, lambda: H.matvec(psi))
        print(f'[matvec] chi={chi} D=5, two components: {t_mv:.3f} ms', flush=True)

        for name, mode in (('pools', False), ('tensors', None)):
            V = krylov._vector_ops(bb, H, psi, mode)
            w = V.enter(psi)
            prev = V.scale(0.5, w)
            beta = V.norm(w)
            t = median_ms(bb, lambda: lanczos_step(V, w, prev, beta))
            print(f'[lanczos] chi={chi} {name}: {t:.3f} ms per step ({t / t_mv:.2f}x a matvec)', flush=True)

        A = sparse.ShiftedLinearOperator(H, 1.5)
        for name, flat in (('pools', True), ('tensors', False)):
            opts = dict(N_max=20, restart=1, res=0.0, N_min=0, flat=flat)

            def cycle():
                g = krylov.GMRES(bb, A, ds.scale(bb, 0.0, psi), psi, opts)
                bb.synchronize()
                t0 = time.perf_counter()
                for k in range(20):
                    g.arnoldi(k)
                    g.apply_givens_rotation(k)
                bb.synchronize()
                return 1e3 * (time.perf_counter() - t0) / 20
            cycle()
            t = statistics.median(cycle() for _ in range(5))
            print(f'[gmres] chi={chi} {name}: {t:.3f} ms per step of a 20-step cycle ({t / t_mv:.2f}x a matvec)', flush=True)

        # 8 independent direct sums: H^k psi, k = 0 .. 7
        vecs = [psi]
        for _ in range(7):
            vecs.append(H.matvec(vecs[-1]))

        def on_pools():
            return sparse.gram_schmidt(bb, vecs)

        def on_tensors():
            usable = krylov._flat_usable
            krylov._flat_usable = lambda *_: False
            try:
                return sparse.gram_schmidt(bb, vecs)
            finally:
                krylov._flat_usable = usable
        assert len(on_pools()) == len(on_tensors()) == 8
        t_p, t_t = [], []
        for _ in range(3):     # alternate the two in one process
            t_p.append(median_ms(bb, on_pools, 3))
            t_t.append(median_ms(bb, on_tensors, 3))
        tp, tt = statistics.median(t_p), statistics.median(t_t)
        print(f'[gram_schmidt] chi={chi} 8 vectors: one call on pools {tp:.3f} ms, host-synchronous loop {tt:.3f} ms '
              f'(pools/loop {tp / tt:.2f})', flush=True)


if __name__ == '__main__':
    main()
