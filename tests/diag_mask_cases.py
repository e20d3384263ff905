"""Seeded cases of the diagonal-tensor / mask tests: legs over Z2, U(1) and U(1) x U(1), and pairs of diagonals with missing
sectors on either or both sides, without blocks at all, with real, complex and boolean entries.  Plain numpy data; a case is
turned into DiagonalTensors of a backend by `to_diag`."""
import numpy as np

from cyten_amd import abelian as ab


def legs():
    z2, u1, u1u1 = ab.Symmetry([2]), ab.Symmetry([0]), ab.Symmetry([0, 0])
    return {
        'z2': ab.Leg(z2, [[0], [1]], [3, 5], +1),
        'u1': ab.Leg(u1, [[-2], [-1], [0], [1], [3]], [1, 4, 7, 2, 66], -1),
        'u1u1': ab.Leg(u1u1, [[-1, 0], [0, -1], [0, 0], [1, 0], [0, 1], [1, 1], [2, -1]], [2, 1, 6, 3, 3, 1, 65], +1),
    }


# which sectors have a block: name -> function of the number of sectors
PRESENCE = {
    'all': lambda n: list(range(n)),
    'none': lambda n: [],
    'even': lambda n: list(range(0, n, 2)),
    'odd': lambda n: list(range(1, n, 2)),
    'first': lambda n: [0],
    'not-first': lambda n: list(range(1, n)),
}
PAIRS = [('all', 'all'), ('even', 'all'), ('all', 'odd'), ('even', 'odd'), ('not-first', 'first'), ('first', 'not-first'), ('even', 'even'),
         ('none', 'all'), ('all', 'none'), ('none', 'none')]


def _values(rng, n, kind):
    if kind == 'bool':
        return rng.random(n) < 0.5
    x = np.round(rng.standard_normal(n), 1)       # (one decimal: ties and exact zeros occur, so eq / ne / le see both answers)
    return x + 1j * np.round(rng.standard_normal(n), 1) if kind == 'complex' else x


def diag(rng, leg, presence, kind):
    """(inds, blocks) of a diagonal on `leg` with blocks in the sectors `presence` names"""
    inds = PRESENCE[presence](leg.nsec)
    return inds, [_values(rng, int(leg.mults[i]), kind) for i in inds]


def pair_cases(kinds=(('real', 'real'), ('complex', 'real'), ('real', 'complex'), ('bool', 'bool'))):
    rng = np.random.default_rng(2024)
    out = []
    for name, leg in legs().items():
        for pa, pb in PAIRS:
            for ka, kb in kinds:
                out.append(dict(id=f'{name}-{pa}-{pb}-{ka}-{kb}', leg=leg, a=diag(rng, leg, pa, ka), b=diag(rng, leg, pb, kb), kinds=(ka, kb)))
    return out


def single_cases(kinds=('real', 'complex', 'bool')):
    rng = np.random.default_rng(2025)
    return [dict(id=f'{name}-{p}-{k}', leg=leg, d=diag(rng, leg, p, k), kind=k)
            for name, leg in legs().items() for p in PRESENCE for k in kinds]


DTYPES = {'real': np.float64, 'complex': np.complex128, 'bool': np.bool_}


def to_diag(bb, leg, d, kind):
    inds, blocks = d
    return ab.DiagonalTensor(leg.symmetry, leg, [bb.as_block(x) for x in blocks], np.array(inds, dtype=np.int64), DTYPES[kind])


def flags_cases():
    """boolean vectors over the whole leg: random ones, all true, all false, and ones that keep or drop WHOLE sectors (where
    ``logical_not`` changes which sectors have blocks)"""
    rng = np.random.default_rng(2026)
    out = []
    for name, leg in legs().items():
        whole = np.zeros(leg.dim, dtype=bool)
        for i in range(0, leg.nsec, 2):
            whole[int(leg.slices[i]):int(leg.slices[i + 1])] = True
        mixed = whole.copy()
        last = slice(int(leg.slices[-2]), int(leg.slices[-1]))
        mixed[last] = rng.random(int(leg.mults[-1])) < 0.5
        for tag, f in (('random', rng.random(leg.dim) < 0.5), ('sparse', rng.random(leg.dim) < 0.1), ('all', np.ones(leg.dim, bool)),
                       ('none', np.zeros(leg.dim, bool)), ('whole-sectors', whole), ('whole-and-part', mixed)):
            out.append(dict(id=f'{name}-{tag}', leg=leg, flags=f))
    return out
