"""Writes tests/golden/ref_integration_surface.json: the interface facts of cyten that tests/test_integration_surface.py
checks the host mirror against, extracted as DATA (names and parameter counts, no source text) from a cyten checkout.

  * the pure virtuals (`virtual ... name(args) ... = 0;`) of ``BlockBackend::Block`` and ``BlockBackend`` in
    include/cyten/block_backend/block_backend.h, with the number of parameters of each;
  * the Array-API attributes ``ArrayApiBlockBackend`` calls on the namespace, on its ``linalg`` and on array objects
    (src/block_backend/array_api.cpp);
  * the operations ``ArrayApiBlockBackend`` leaves NotImplemented (same file).

    python scripts/make_integration_surface_golden.py PATH_TO_CYTEN_CHECKOUT
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'ref_integration_surface.json')
HEADER = 'include/cyten/block_backend/block_backend.h'
ARRAY_API = 'src/block_backend/array_api.cpp'


def pure_virtuals(text):
    """[(name, n_params)] of the `virtual ... name(args) ... = 0;` declarations in a class body"""
    out = []
    for m in re.finditer(r'virtual\s+[^;{}]*?\b(operator\s*[^\s(]+|[A-Za-z_]\w*)\s*\(([^;{}]*?)\)\s*(?:const\s*)?=\s*0\s*;', text, re.S):
        name = re.sub(r'\s+', '', m.group(1))
        args = m.group(2).strip()
        depth, n = 0, (1 if args else 0)
        for ch in args:
            depth += ch in '<('
            depth -= ch in '>)'
            n += (ch == ',' and depth == 0)
        out.append((name, n))
    return out


def extract(ref):
    text = open(os.path.join(ref, HEADER)).read()
    i_block = text.index('class Block : public std::enable_shared_from_this<Block>')
    i_scalar = text.index('/// Holds a single scalar value', i_block)
    src = open(os.path.join(ref, ARRAY_API)).read()
    api_names = set(re.findall(r'api_\.attr\("(\w+)"\)(?!\.attr)', src)) | set(re.findall(r'api\(\)\.attr\("(\w+)"\)', src))
    return {
        '_doc': 'Interface facts of cyten for tests/test_integration_surface.py, extracted as data by '
                'scripts/make_integration_surface_golden.py: pure virtuals [name, number of parameters] of BlockBackend::Block '
                f'and BlockBackend ({HEADER}); Array-API attributes ArrayApiBlockBackend uses on the namespace, its linalg and '
                f'array objects, and the operations it leaves NotImplemented ({ARRAY_API}).',
        'block_virtuals': pure_virtuals(text[i_block:i_scalar]),
        'backend_virtuals': pure_virtuals(text[i_scalar:]),
        'array_api_namespace': sorted(api_names),
        'array_api_linalg': sorted(set(re.findall(r'api_\.attr\("linalg"\)\.attr\("(\w+)"\)', src))),
        'array_api_array': sorted(set(re.findall(r'(?:arr_|obj\([a-z_]*\)|\ba|\bb)\.attr\("(\w+)"\)', src))),
        'array_api_not_implemented': sorted(set(re.findall(r'NotImplemented\("ArrayApiBlockBackend does not support (\w+)\.', src))),
    }


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with open(OUT, 'w') as f:
        json.dump(extract(sys.argv[1]), f, indent=1)
        f.write('\n')
    print(OUT)
