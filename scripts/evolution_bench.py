"""Krylov time evolution on the device (two-site TDVP step): the H_eff matvec of a real operator on a real theta and on a
complex theta, and LanczosEvolution for delta = -0.1i, against the numpy per-block path on the host.

    python scripts/evolution_bench.py [chi ...]        (default 1024 4096; D = 5)

Runs against older trees too: what they lack (LanczosEvolution) is reported as missing."""
import sys
import time

import numpy as np

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
from cyten_amd.block_backend import HipBlockBackend  # noqa: E402
from cyten_amd import krylov, workloads as wl  # noqa: E402
from helpers import to_device_tensor  # noqa: E402
from numpy_backend import NumpyGroupedBackend  # noqa: E402


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


def main():
    bb = HipBlockBackend('cuda:0')
    nbk = NumpyGroupedBackend()
    chis = [int(x) for x in sys.argv[1:]] or [1024, 4096]
    for chi in chis:
        cfg = wl.config_heff(chi, 5, seed=11)
        rng = np.random.default_rng(12)
        theta_c = [b + 1j * rng.standard_normal(b.shape) for b in cfg['theta'].blocks]
        dev = {k: to_device_tensor(bb, v) for k, v in cfg.items()}
        real_theta = cfg['theta'].blocks
        cfg['theta'].blocks = theta_c
        dev_c = to_device_tensor(bb, cfg['theta'])
        cfg['theta'].blocks = real_theta
        H = krylov.HEffective(bb, dev['LP'], dev['W1'], dev['W2'], dev['RP'])
        t_real = best_ms(bb, lambda: H.matvec(dev['theta']))
        t_cplx = best_ms(bb, lambda: H.matvec(dev_c))
        print(f'[matvec] chi={chi} D=5: real {t_real:.2f} ms, complex theta {t_cplx:.2f} ms '
              f'(ratio {t_cplx / t_real:.2f})', flush=True)
        if hasattr(krylov, 'LanczosEvolution'):
            opts = dict(N_max=20)
            krylov.LanczosEvolution(bb, H, dev['theta'], opts).run(-0.1j)    # (warm: recordings, plans)
            bb.synchronize()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                psi, N = krylov.LanczosEvolution(bb, H, dev['theta'], opts).run(-0.1j)
                bb.synchronize()
                ts.append(time.perf_counter() - t0)
            t_ev = 1e3 * min(ts)
            print(f'[evolution] chi={chi}: LanczosEvolution(-0.1i) N={N}, {t_ev:.1f} ms, {t_ev / N:.2f} ms per Krylov step '
                  f'({t_ev / N / t_real:.2f}x a real matvec)', flush=True)
        else:
            print(f'[evolution] chi={chi}: LanczosEvolution missing in this tree', flush=True)
        if chi <= 1024:   # (the host path at chi=4096 takes minutes per matvec)
            cpu = {k: to_device_tensor(nbk, v) for k, v in cfg.items()}
            Hc = krylov.HEffective(nbk, cpu['LP'], cpu['W1'], cpu['W2'], cpu['RP'])
            Hc.matvec(cpu['theta'])
            t0 = time.perf_counter()
            Hc.matvec(cpu['theta'])
            t_cpu = 1e3 * (time.perf_counter() - t0)
            print(f'[host] chi={chi}: numpy per-block real matvec {t_cpu:.0f} ms ({t_cpu / t_real:.0f}x the device)', flush=True)


if __name__ == '__main__':
    main()
