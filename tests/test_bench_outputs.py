"""bench.py's result line and --dump-outputs: what the timed path computed in its last step, written as float64 .npy files
within the byte budget (CPU: the writer on host arrays; GPU: a plain run end to end)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

NAMES = ('S', 'kept_per_sector', 'sector_shapes', 'truncation', 'triplets', 'U', 'Vh')


class _HostBackend:
    """stands in for the device backend: the 'blocks' are host arrays already"""

    @staticmethod
    def to_numpy(x):
        return np.asarray(x)


def _step(rng, shapes, kept):
    res = {'shapes': shapes, 'kept_n': np.array(kept), 'err': 0.25, 'new_norm': 0.75, 'kept': []}
    for (m, n), c in zip(shapes, kept):
        res['kept'].append((rng.standard_normal((m, c)), np.sort(rng.random(c))[::-1], rng.standard_normal((c, n))))
    return res


def _load(d):
    return {k: np.load(os.path.join(d, k + '.npy')) for k in NAMES}


def _check_triplets(res, out):
    """every written U column / Vh row is the one of the triplet `triplets` names"""
    kept = res['kept_n']
    starts = np.concatenate([[0], np.cumsum(kept)])
    ou = ov = 0
    for j in out['triplets'].astype(np.int64):
        u = int(np.searchsorted(starts, j, side='right') - 1)
        U, S, Vh = res['kept'][u]
        m, n = res['shapes'][u]
        assert np.array_equal(out['U'][ou:ou + m], U[:, j - starts[u]])
        assert np.array_equal(out['Vh'][ov:ov + n], Vh[j - starts[u], :])
        assert out['S'][j] == S[j - starts[u]]
        ou, ov = ou + m, ov + n
    assert ou == out['U'].size and ov == out['Vh'].size


def test_dump_outputs_writes_every_triplet_when_it_fits(tmp_path):
    res = _step(np.random.default_rng(3), [(5, 4), (9, 7), (3, 3)], [2, 0, 3])
    bench.dump_outputs(_HostBackend(), res, str(tmp_path))
    out = _load(str(tmp_path))
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out['triplets'], np.arange(5)) and np.array_equal(out['kept_per_sector'], [2, 0, 3])
    assert np.array_equal(out['truncation'], [0.25, 0.75]) and np.array_equal(out['sector_shapes'], [(5, 4), (9, 7), (3, 3)])
    _check_triplets(res, out)


def test_dump_outputs_samples_whole_triplets_within_the_budget(tmp_path):
    res = _step(np.random.default_rng(4), [(300, 280), (200, 260), (90, 90)], [120, 90, 40])
    budget = 200_000                                        # the whole set needs about 1 MB
    bench.dump_outputs(_HostBackend(), res, str(tmp_path / 'a'), budget=budget)
    bench.dump_outputs(_HostBackend(), res, str(tmp_path / 'b'), budget=budget)
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert sum(os.path.getsize(tmp_path / 'a' / (k + '.npy')) for k in NAMES) <= budget
    assert 0 < a['triplets'].size < 250 and np.all(np.diff(a['triplets']) > 0)
    assert a['S'].size == 250                               # every kept singular value, sampled or not
    for k in NAMES:                                         # the same sample for the same arguments
        assert np.array_equal(a[k], b[k])
    _check_triplets(res, a)


def test_steps_must_be_positive():
    assert bench.parse(['--steps', '3']).steps == 3 and not bench.parse([]).full
    with pytest.raises(SystemExit):
        bench.parse(['--steps', '0'])


@pytest.mark.gpu
def test_plain_bench_run_dumps_its_last_step(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--chi', '256', '--steps', '3', '--warmup', '1',
           '--dump-outputs', str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.strip().splitlines() if x.startswith('{')][-1])
    assert line['steps'] == 3 and line['ms_per_step'] > 0 and line['dtype'] == 'f64' and line['higher_is_better'] is True
    assert 'cpu_baseline' not in line and 'roofline_u1u1' not in line           # a plain run measures only its steps
    out = _load(str(tmp_path))
    assert all(a.dtype == np.float64 for a in out.values())
    assert out['S'].size == line['truncation']['kept'] == out['kept_per_sector'].sum()
    assert np.array_equal(out['triplets'], np.arange(out['S'].size))            # chi=256 fits the budget whole
    assert abs(out['truncation'][0] - line['truncation']['err']) <= 1e-12 * max(1.0, line['truncation']['new_norm'])
    # the factors are the truncated SVD: singular values descending inside each sector, orthonormal singular vectors
    ou = ov = start = 0
    for c, (m, n) in zip(out['kept_per_sector'].astype(np.int64), out['sector_shapes'].astype(np.int64)):
        U = out['U'][ou:ou + c * m].reshape(c, m).T
        Vh = out['Vh'][ov:ov + c * n].reshape(c, n)
        assert np.all(np.diff(out['S'][start:start + c]) <= 0)
        assert np.abs(U.T @ U - np.eye(c)).max(initial=0.0) <= 1e-10 and np.abs(Vh @ Vh.T - np.eye(c)).max(initial=0.0) <= 1e-10
        ou, ov, start = ou + c * m, ov + c * n, start + c
    assert ou == out['U'].size and ov == out['Vh'].size and start > 0
