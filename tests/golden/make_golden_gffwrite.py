"""Record what the REFERENCE's own convert_gff prints: tests/golden/gffwrite.json.

Runs only where the reference is installed (see make_golden.py, whose lib2to3
copy this imports); the reference functions (genome_tools.py:527-545,
genome.py:228-238, 616-645, 733-778) run unchanged, and nothing of their
program text is stored: only inputs, stdout, exception names and each case's
note of its path.

The copy runs under Python 3, which differs from the Python 2 target in three
places these functions touch; all are handled here, not in the copy.

  * ``open``: text mode would translate line ends and decode UTF-8.  The copied
    ensure_file gets a shadow that opens with ``newline='\\n'`` and
    ``encoding='latin-1'``.
  * ``str(float)``: Python 3 prints ``repr``.  Every numeric score of the cases
    has at most 12 significant digits, where both spellings agree; this is
    asserted for every score column before a case is run.
  * dict iteration order: ``out`` is the reference's stdout as it came, that is
    the 'insertion' record.  The Python 2 order is pinned by the reference's own
    three goldens instead (test_data/test_suite.py:15-17), whose cksum and size
    are stored under ``cksums``; none of those large outputs is.

Per case and output format: ``out``, ``exc``; per case ``gff`` and ``path``.

Usage:  python tests/golden/make_golden_gffwrite.py
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
import gffwrite_expect as gx  # noqa: E402


def check_scores(gff):
    for line in gff.split('\n'):
        cols = line.split('\t')
        if len(cols) == 9 and not line.startswith('#'):
            try:
                value = float(cols[5])
            except ValueError:
                continue
            assert gx.py2_float_str(value) == repr(value), cols[5]


def main():
    make_golden.reference_module()
    import genome_tools as tools
    import magot_smallfuncs as small
    small.open = lambda path, *a, **k: builtins.open(path, newline='\n', encoding='latin-1')
    gold = {'cksums': [[list(cmd), list(pair)] for cmd, pair in gx.CKSUMS], 'cases': {}}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'in.gff')
        for name, case in gx.cases().items():
            check_scores(case['gff'])
            with open(path, 'wb') as fh:
                fh.write(case['gff'].encode('latin-1'))
            runs = {}
            for fmt in gx.FORMATS:
                _, exc, out = make_golden.call(lambda: tools.convert_gff(path, 'gff3', fmt))
                runs[fmt] = {'out': out, 'exc': exc}
                print(name, fmt, exc, len(out), flush=True)
            gold['cases'][name] = {'gff': case['gff'], 'path': case['path'], 'runs': runs}
    with open(os.path.join(HERE, 'gffwrite.json'), 'w') as fh:
        json.dump(gold, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
