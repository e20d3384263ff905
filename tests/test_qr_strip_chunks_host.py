"""The chunk arithmetic of the row-split QR strips (``csrc/qr_strip_chunks.h``), checked on the host under ASan and UBSan.

``qr_strip_chunks.cpp`` includes only that header.  A panel step writes one 32 x 32 partial per chunk into a workspace
that was sized earlier from a different expression (``bqr_strip_slots``): for every strip of 1 ... 4096 rows and every
chunk size the switches can select it requires that the chunks cover the rows exactly once, in ascending order, start at
multiples of 16, are never empty and never outnumber the slots; ``choose_chunk_rows`` is pinned by strip lists worked
out by hand.
"""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _compiler() -> str:
    exe = shutil.which('c++')
    if exe:
        return exe
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    for cand in (Path(hipcc).resolve().parent / 'clang++', Path(hipcc).resolve().parent.parent / 'llvm' / 'bin' / 'clang++',
                 Path(hipcc).resolve().parent.parent / 'lib' / 'llvm' / 'bin' / 'clang++'):
        if cand.exists():
            return str(cand)
    raise RuntimeError('neither a host c++ nor the clang++ beside hipcc was found')


def test_qr_strip_chunks(tmp_path):
    exe = tmp_path / 'qr_strip_chunks'
    cmd = [_compiler(), '-std=c++17', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I', str(ROOT / 'cyten_amd' / 'csrc'), str(ROOT / 'tests' / 'qr_strip_chunks.cpp'), '-o', str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, f'{" ".join(cmd)}\n{res.stdout}\n{res.stderr}'
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, f'{res.stdout}\n{res.stderr}'
    assert 'no mismatch' in res.stdout, res.stdout
