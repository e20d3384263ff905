"""Thick-restart Lanczos on the device on the H_eff workload of scripts/direct_sum_bench.py (config_heff, D = 5):

(a) the basis rotation Y = V S of a restart: krylov._FlatOps.rotate -- ONE cyb_basis_rotate_f64 call, in place -- against l
    calls of krylov._FlatOps.combine on the same pools (the route the library had before), for (m, l) = (24, 12) and (40, 22).
    Call time: host clock around one rotation that ends in a device synchronise.  Device time: 20 rotations enqueued back to
    back, one synchronise, divided by 20 (kernel time proper: rocprofv3 --kernel-trace --stats on `--rotation-only`, in a run
    of its own).  Bytes: (m + l) n words for the kernel; the byte model predicts kernel / combine = (m + l) / (l (m + 1)).
(b) LanczosEigenpairs(num_ev=4) against four successive LanczosGroundState solves on ProjectedLinearOperator (the only route
    to excited states before), both to the same TRUE residual |H y - E y|: matvec counts and wall time.  A solve of that
    route is restarted Lanczos with the same bounded memory: cycles of 20 steps with full reorthogonalisation (P_tol = 0: a
    cycle is not cut short by the two-vector gap estimate of a nearly converged start), each from the result of the one
    before, until the residual is that of the thick-restart run -- its counts are multiples of 20.

    python scripts/eigenpairs_bench.py [--rotation-only] [chi ...]     (default 1024 4096; (b) runs for chi <= 1024)

Medians of 7 after a warm-up, profiler off, the two routes alternating in one process.  One line per figure."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
from cyten_amd.block_backend import HipBlockBackend  # noqa: E402
from cyten_amd import krylov, sparse, workloads as wl  # noqa: E402
from helpers import to_device_tensor  # noqa: E402

BACK_TO_BACK = 20
STATES_CHI_MAX = 1024


def timed_ms(bb, fn):
    t0 = time.perf_counter()
    fn()
    bb.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def median_ms(bb, fn, reps=7):
    fn()
    bb.synchronize()
    return statistics.median(timed_ms(bb, fn) for _ in range(reps))


def rotation(bb, V, w, chi):
    n = V.total
    rng = np.random.default_rng(5)
    for m, l in ((24, 12), (40, 22)):
        pools = [V.scale(1.0 + 0.01 * j, w) for j in range(m)]
        # orthonormal columns, halved: repeated in-place rotations of the same pools stay bounded
        S = 0.5 * np.linalg.qr(rng.standard_normal((m, m)))[0][:, :l]

        def rotate():
            V.rotate(pools, S)

        def combine():
            return [V.combine([float(c) for c in S[:, i]], pools) for i in range(l)]

        def many(fn):
            def run():
                for _ in range(BACK_TO_BACK):
                    fn()
            return run
        call_r, call_c, dev_r, dev_c = [], [], [], []
        for _ in range(3):          # alternate the two routes
            call_r.append(median_ms(bb, rotate))
            call_c.append(median_ms(bb, combine))
            dev_r.append(median_ms(bb, many(rotate), 3) / BACK_TO_BACK)
            dev_c.append(median_ms(bb, many(combine), 3) / BACK_TO_BACK)
        call_r, call_c, dev_r, dev_c = (statistics.median(x) for x in (call_r, call_c, dev_r, dev_c))
        words = (m + l) * n
        model = (m + l) / (l * (m + 1))
        print(f'[rotate] chi={chi} n={n} (m, l)=({m}, {l}): one call {call_r:.3f} ms, back to back {dev_r:.3f} ms = '
              f'{8e-9 * words / dev_r:.2f} TB/s over (m + l) n words | {l} combine calls {call_c:.3f} ms, back to back {dev_c:.3f} ms | '
              f'rotate / combine: calls {call_r / call_c:.3f}, back to back {dev_r / dev_c:.3f}, byte model {model:.3f}', flush=True)
        del pools


def true_residual(T, H, E, y):
    return T.norm(T.lincomb(1.0, H.matvec(y), -float(E), y))


def excited_states(bb, H, theta, chi, num_ev=4, tol=1e-8):
    T = krylov._TensorOps(bb, H)
    out = {}

    def thick():
        solver = krylov.LanczosEigenpairs(bb, H, theta, dict(num_ev=num_ev, which='SA', tol=tol, max_restarts=500))
        Es, vecs, N = solver.run()
        out['thick'] = (Es, vecs, N, solver.restarts)

    def successive():
        found, Es, matvecs, cycles = [], [], 0, 0
        for _ in range(num_ev):
            op = sparse.ProjectedLinearOperator(H, found, project_operator=True) if found else H
            psi = theta
            for _ in range(200):
                E, psi, N = krylov.LanczosGroundState(bb, op, psi, dict(N_max=20, reortho=True, P_tol=0.0)).run()
                matvecs += N
                cycles += 1
                if true_residual(T, op, E, psi) <= out['target']:      # (one more matvec per cycle: not counted)
                    break
            found.append(psi)
            Es.append(E)
        out['successive'] = (np.array(Es), found, matvecs, cycles)

    thick()
    Es, vecs, N, restarts = out['thick']
    res = [true_residual(T, H, E, y) for E, y in zip(Es, vecs)]
    out['target'] = max(res)
    successive()
    t_thick, t_succ = [], []
    for _ in range(3):
        t_thick.append(timed_ms(bb, thick))
        t_succ.append(timed_ms(bb, successive))
    Es2, found, N2, cycles = out['successive']
    res2 = [true_residual(T, H, E, y) for E, y in zip(Es2, found)]
    print(f'[states] chi={chi} num_ev={num_ev} tol={tol:g}: LanczosEigenpairs {N} matvecs, {restarts} restarts, '
          f'{statistics.median(t_thick):.1f} ms, true residuals <= {max(res):.2e} | {num_ev} x restarted LanczosGroundState on P H P '
          f'{N2} matvecs (+{cycles} residual checks) in {cycles} cycles, {statistics.median(t_succ):.1f} ms, true residuals <= '
          f'{max(res2):.2e} | matvecs {N / N2:.2f}, time {statistics.median(t_thick) / statistics.median(t_succ):.2f}; '
          f'largest |dE| between the routes {np.abs(Es - Es2).max():.2e}, E = {np.array2string(Es, precision=6)}', flush=True)


def main():
    args = sys.argv[1:]
    rotation_only = '--rotation-only' in args
    chis = [int(x) for x in args if not x.startswith('--')] or [1024, 4096]
    bb = HipBlockBackend('cuda:0')
    for chi in chis:
        cfg = wl.config_heff(chi, 5, seed=11)
        dev = {k: to_device_tensor(bb, v) for k, v in cfg.items()}
        H = krylov.HEffective(bb, dev['LP'], dev['W1'], dev['W2'], dev['RP'])
        theta = dev['theta']
        V = krylov._vector_ops(bb, H, theta, False)
        w = V.enter(theta)
        t_mv = median_ms(bb, lambda: H.matvec(theta))
        print(f'[matvec] chi={chi} D=5: {t_mv:.3f} ms, pool of {V.total} doubles', flush=True)
        rotation(bb, V, w, chi)
        if not rotation_only and chi <= STATES_CHI_MAX:
            excited_states(bb, H, theta, chi)


if __name__ == '__main__':
    main()
