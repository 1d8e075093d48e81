"""Record what the REFERENCE's own purge_overlaps prints and annotation_overlap
returns: tests/golden/overlap.json.

Runs only where the reference is installed (see make_golden.py, whose
lib2to3 copy this imports); the reference functions (genome_tools.py:548-568,
annotation_funcs.py:13-30) run unchanged, and nothing of their program text is
stored: only inputs, outputs and exception names.

The copy runs under Python 3, which differs from the Python 2 target in two
places these functions touch; both are handled here, not in the copy:

  * ``open``: text mode would translate line ends and decode UTF-8.  The
    shadow opens with ``newline='\\n'`` (lines end at LF only, nothing is
    translated) and ``encoding='latin-1'`` (one character per byte).
  * dict iteration order.  annotation_overlap's result follows the second
    dict's; it is recorded twice, with that dict filled in the given order
    ('insertion') and in the order a Python 2 dict of those keys iterates
    (oracle.magot_oracle.py2_dict_order; 'py2').

Per purge case: ``first`` and ``second`` (the files' bytes as latin-1), ``out``
(stdout, what came before an exception included), ``exc`` (exception name or
null) and ``path`` (the case's own note of the path it is meant for: 'native',
or why the planner must decline).  Per overlap case: the two annotation sets
and dict names (tests/overlap_expect.py: overlap_cases), and per order ``out``
(the returned list or null) and ``exc``.

Usage:  python tests/golden/make_golden_overlap.py
"""

import builtins
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
import overlap_expect as oe  # noqa: E402
from oracle import magot_oracle as mo  # noqa: E402


def shadow(tools):
    tools.open = lambda path, *a, **k: builtins.open(path, newline='\n', encoding='latin-1')


def main():
    ref = make_golden.reference_module()
    import genome_tools as tools
    import annotation_funcs as funcs
    shadow(tools)
    purge = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, 'first.gff'), os.path.join(tmp, 'second.gff')]
        for name, (first, second, path) in oe.purge_cases().items():
            for p, data in zip(paths, (first, second)):
                with open(p, 'wb') as fh:
                    fh.write(data)
            _, exc, text = make_golden.call(lambda: tools.purge_overlaps(*paths))
            purge[name] = {'first': first.decode('latin-1'), 'second': second.decode('latin-1'),
                           'out': text, 'exc': exc, 'path': path}
            print(name, exc, len(text), flush=True)
    overlap = {}
    for name, (spec1, which1, spec2, which2) in oe.overlap_cases().items():
        rec = {'first': spec1, 'first_dict': which1, 'second': spec2, 'second_dict': which2}
        for order in ('insertion', 'py2'):
            d1 = oe.build_features(ref, spec1, which1)
            d2 = oe.build_features(ref, spec2, which2)
            if order == 'py2':
                d1 = {k: d1[k] for k in mo.py2_dict_order(list(d1))}
                d2 = {k: d2[k] for k in mo.py2_dict_order(list(d2))}
            res, exc, text = make_golden.call(lambda: funcs.annotation_overlap(d1, d2))
            assert text == '', text
            rec[order] = {'out': res, 'exc': exc}
        overlap[name] = rec
        print(name, rec['insertion']['exc'], rec['insertion']['out'], flush=True)
    with open(os.path.join(HERE, 'overlap.json'), 'w') as fh:
        json.dump({'purge': purge, 'overlap': overlap}, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
