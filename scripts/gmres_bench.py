"""GMRES on the device: the H_eff matvec, one 20-step GMRES cycle on float64 pools, and the fused
classical Gram-Schmidt step (cyb_gram_schmidt_f64, passes=2) against the modified Gram-Schmidt sequence of single
`inner` / `lincomb` calls it replaces, alternating in one process.

    python scripts/gmres_bench.py [chi ...]        (default 1024 4096; D = 5, the config_heff operator)

The fused step is timed with a host clock around repeated launches that end in a device synchronise (no coefficient copy);
its bytes are (3m + 5) n words from the shapes.  Kernel-level times come from a separate rocprofv3 --kernel-trace --stats
run of this script."""
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
from cyten_amd.block_backend import HipBlockBackend  # noqa: E402
from cyten_amd import abelian as ab, krylov, sparse, workloads as wl  # noqa: E402
from helpers import to_device_tensor  # noqa: E402


def best_ms(bb, fn, reps=5):
    fn()
    bb.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        bb.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts)


def mgs(V, basis, w):
    """The MGS sequence of earlier Arnoldi code: per basis vector one inner (with its host copy) and one lincomb."""
    for v in basis:
        c = V.inner(v, w)
        w = V.lincomb(1.0, w, -c, v)
    return w, V.norm(w)


def main():
    bb = HipBlockBackend('cuda:0')
    chis = [int(x) for x in sys.argv[1:]] or [1024, 4096]
    for chi in chis:
        cfg = wl.config_heff(chi, 5, seed=11)
        dev = {k: to_device_tensor(bb, v) for k, v in cfg.items()}
        H = krylov.HEffective(bb, dev['LP'], dev['W1'], dev['W2'], dev['RP'])
        theta = dev['theta']
        t_mv = best_ms(bb, lambda: H.matvec(theta))
        print(f'[matvec] chi={chi} D=5: {t_mv:.3f} ms', flush=True)

        # one GMRES cycle of 20 Arnoldi steps (matvec + fused CGS2 + Givens), res=0 so that no step ends it
        A = sparse.ShiftedLinearOperator(H, 1.5)
        opts = dict(N_max=20, restart=1, res=0.0, N_min=0)

        def cycle():
            g = krylov.GMRES(bb, A, ab.scale(bb, 0.0, theta), theta, opts)
            bb.synchronize()
            t0 = time.perf_counter()
            for k in range(20):
                g.arnoldi(k)
                g.apply_givens_rotation(k)
            bb.synchronize()
            return 1e3 * (time.perf_counter() - t0), g
        cycle()
        t_cyc = min(cycle()[0] for _ in range(3))
        print(f'[gmres] chi={chi}: 20-step cycle {t_cyc:.2f} ms, {t_cyc / 20:.3f} ms per step '
              f'({t_cyc / 20 / t_mv:.2f}x a matvec)', flush=True)

        # the orthogonalisation alone: fused CGS2 vs the MGS sequence on the same float64 pools
        _, g = cycle()
        V = g.V
        n = V.total
        for m in (1, 11, 21):
            basis = [bb.ctx.empty(n).normal_() for _ in range(m)]
            w0 = bb.ctx.empty(n).normal_()
            w = w0.clone()
            out = bb.ctx.empty(m + 1)
            reps = 20

            def fused():
                for _ in range(reps):
                    V._gs(basis, w, 2, out)

            def seq():
                for _ in range(reps):
                    mgs(V, basis, w0)
            t_f, t_s = [], []
            fused()
            seq()
            for _ in range(3):     # alternate the two in one process
                t_f.append(best_ms(bb, fused, 1) / reps)
                t_s.append(best_ms(bb, seq, 1) / reps)
            tf, ts = min(t_f), min(t_s)
            nbytes = (3 * m + 5) * n * 8
            print(f'[ortho] chi={chi} m={m}: n={n}, fused CGS2 {tf:.3f} ms ({nbytes / tf / 1e9:.2f} TB/s on {nbytes / 1e6:.1f} MB), '
                  f'MGS sequence {ts:.3f} ms (fused/MGS {tf / ts:.2f})', flush=True)


if __name__ == '__main__':
    main()
