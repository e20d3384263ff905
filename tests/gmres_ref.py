"""Dense numpy restatement of the reference's restarted GMRES (src/tensors/krylov_based.cpp:358-530: constructor :358-387,
run :405-451, arnoldi :453-469, apply_givens_rotation :471-487, givens_rotation :489-498, backsolve :500-513, reset
:515-530) with the two deviations cyten_amd.krylov.GMRES documents: the unitary Givens rotation
[[conj(c), conj(s)], [-s, c]] with t = sqrt(|v1|^2 + |v2|^2), and a zero new Krylov vector ending the cycle as converged.
Orthogonalisation by modified Gram-Schmidt, as the reference."""
import numpy as np


def gmres_dense(matvec, x, b, N_min=5, N_max=20, restart=10, res=1e-8):
    """(x, rel_residual, total_error, total_iters) for numpy vectors."""
    x = np.array(x, dtype=np.result_type(x, b, np.float64))
    b_norm = np.linalg.norm(b)
    denom = b_norm if b_norm != 0.0 else 1.0

    def start(x):
        r = b - matvec(x)
        r_norm = np.linalg.norm(r)
        return r_norm, [r / r_norm if r_norm > 0 else r]

    r_norm, qs = start(x)
    total_error = [[r_norm / denom]]
    total_iters = []
    if total_error[0][0] < res:
        return x, total_error[0][0], total_error, total_iters
    for _ in range(restart):
        H = np.zeros((N_max + 1, N_max), dtype=np.complex128)
        cs = np.zeros(N_max, dtype=np.complex128)
        sn = np.zeros(N_max, dtype=np.complex128)
        e1 = np.zeros(N_max + 1, dtype=np.complex128)
        e1[0] = r_norm
        converged, performed = False, 0
        for k in range(N_max):
            q = matvec(qs[-1])
            for i in range(k + 1):
                H[i, k] = np.vdot(qs[i], q)
                q = q - H[i, k] * qs[i]
            h_next = np.linalg.norm(q)
            H[k + 1, k] = h_next
            if h_next > 0:
                q = q / h_next
            qs.append(q)
            for i in range(k):
                t = np.conj(cs[i]) * H[i, k] + np.conj(sn[i]) * H[i + 1, k]
                H[i + 1, k] = -sn[i] * H[i, k] + cs[i] * H[i + 1, k]
                H[i, k] = t
            v1, v2 = H[k, k], H[k + 1, k]
            t = np.sqrt(abs(v1) ** 2 + abs(v2) ** 2)
            cs[k], sn[k] = (v1 / t, v2 / t) if t > 0 else (1.0, 0.0)
            H[k, k] = np.conj(cs[k]) * H[k, k] + np.conj(sn[k]) * H[k + 1, k]
            H[k + 1, k] = 0
            e1[k + 1] = -sn[k] * e1[k]
            e1[k] = np.conj(cs[k]) * e1[k]
            error = abs(e1[k + 1]) / denom
            total_error[-1].append(error)
            performed = k + 1
            if (error < res and k >= N_min) or h_next == 0.0:
                converged = True
                break
        total_iters.append(performed)
        y = np.zeros(performed, dtype=np.complex128)
        for i in range(performed - 1, -1, -1):
            y[i] = (e1[i] - H[i, i + 1:performed] @ y[i + 1:]) / H[i, i]
        upd = sum(y[i] * qs[i] for i in range(performed))
        x = x + (upd.real if not np.iscomplexobj(x) else upd)
        if converged:
            break
        r_norm, qs = start(x)
        total_error.append([r_norm / denom])
    rel = np.linalg.norm(matvec(x) - b) / (b_norm if b_norm != 0.0 else 1.0)
    return x, rel, total_error, total_iters


def projected_dense(Hm, ortho, vec, project_operator=True, penalty=None):
    """The sequential projection of sparse.cpp:294-327 on dense vectors (ortho vectors need not be orthonormal)."""
    res = vec.copy()
    coeffs = []
    if project_operator:
        for o in ortho:
            c = np.vdot(o, res)
            coeffs.append(c)
            res = res - c * o
    else:
        coeffs = [np.vdot(o, res) for o in ortho]
    res = Hm @ res
    if project_operator:
        for o in ortho:
            res = res - np.vdot(o, res) * o
    if penalty is not None:
        for o, c in zip(ortho, coeffs):
            res = res + penalty * c * o
    return res
