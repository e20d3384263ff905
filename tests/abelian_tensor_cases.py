"""Seeded inputs shared by the CPU and GPU tests of the tensor-level operations conj / dagger / scale_axis / partial_trace /
trace_full / dense conversion: plain-data tensors (cyten_amd.workloads.TensorSpec) with the traced pairs.  Leg patterns after
the reference's ``test_partial_trace`` parametrisation; ``x*`` = ``wl.flip(x)``, ``x^`` = the dual space written with the SAME
sign (negated sectors, so the two legs of the pair list their sectors in different orders)."""
import numpy as np

import abelian_tensor_ref as ref
from cyten_amd import workloads as wl

SYMMETRIES = [(0,), (3,), (0, 2)]        # U(1), Z3, U(1) x Z2
PATTERNS = ['same_side', 'scalar', 'one_pair', 'two_pairs']


def _leg(rng, moduli, n, sign):
    if moduli == (0,):
        qs = np.sort(rng.choice(np.arange(-2, 3), size=n, replace=False))
        return wl.make_leg(moduli, qs[:, None], rng.integers(1, 5, n), sign)
    if moduli == (3,):
        return wl.make_leg(moduli, np.arange(3)[:n, None], rng.integers(1, 4, n), sign)
    secs = [(q, z) for q in (-1, 0, 1) for z in (0, 1)]
    pick = rng.choice(len(secs), size=n, replace=False)
    return wl.make_leg(moduli, np.array(secs)[pick], rng.integers(1, 4, n), sign)


def dual_same_sign(leg, moduli):
    return wl.make_leg(moduli, -leg.sectors, leg.mults, leg.sign)


def trace_cases(seed=21):
    """[dict(name, moduli, tensor, pairs)], 4 leg patterns x 3 symmetries.  In every case at least one block is off the
    diagonal (skipped) and at least one result block is the sum of two or more source blocks: asserted here, so that a
    reseed cannot lose either silently."""
    rng = np.random.default_rng(seed)
    out = []
    for moduli in SYMMETRIES:
        a, b, c, d = _leg(rng, moduli, 3, +1), _leg(rng, moduli, 3, +1), _leg(rng, moduli, 3, -1), _leg(rng, moduli, 2, -1)
        patterns = [
            ('same_side', [a, b, dual_same_sign(a, moduli), c, d], 3, [(0, 2)]),
            ('scalar', [a, b, wl.flip(b), wl.flip(a)], 2, [(0, 3), (1, 2)]),
            ('one_pair', [a, wl.flip(c), wl.flip(b), wl.flip(a)], 2, [(0, 3)]),
            ('two_pairs', [a, b, wl.flip(b), wl.flip(a), c, wl.flip(c)], 3, [(0, 3), (1, 2)]),
        ]
        for name, legs, n_cod, pairs in patterns:
            t = wl.random_tensor(moduli, legs, rng, num_codomain=n_cod, fill=0.85)
            _, stats = ref.partial_trace(t, pairs)
            assert stats['off'] >= 1, f'{moduli} {name}: no block is off the diagonal'
            assert stats['multi'] >= 1, f'{moduli} {name}: no result block receives two source blocks'
            out.append(dict(name=name, moduli=moduli, tensor=t, pairs=pairs, stats=stats))
    return out


CASE_IDS = [f'{"x".join("U1" if m == 0 else f"Z{m}" for m in moduli)}-{name}' for moduli in SYMMETRIES for name in PATTERNS]


def case_tensor(case, cplx, seed=5):
    """the tensor of a case, with seeded imaginary parts if `cplx`"""
    t = case['tensor']
    return ref.complexified(t, np.random.default_rng(seed)) if cplx else t


def diagonal_values(leg, seed=3, drop_sector=None):
    """positive values over a leg (singular-value like), one of them tiny; `drop_sector`: that sector is left out of the
    returned {sector: block} dictionary"""
    rng = np.random.default_rng(seed)
    vals = rng.random(int(leg.mults.sum())) + 0.1
    vals[0] = 1e-14
    blocks = ref.diagonal_blocks(leg, vals)
    if drop_sector is not None:
        blocks.pop(drop_sector)
    return vals, blocks
