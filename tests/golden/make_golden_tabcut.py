"""Record what the REFERENCE's own tab2fasta and repeatmasker2augustushints
print: tests/golden/tabcut.json.

Runs only where the reference is installed (see make_golden.py, whose lib2to3
copy this imports); both reference functions (genome_tools.py:345-346 over
magot_smallfuncs.py:12-18, and genome_tools.py:449-454) run unchanged, and
nothing of their program text is stored: only inputs, stdout and exception
names.

The copy runs under Python 3, whose text-mode ``open`` would translate line
ends and decode UTF-8.  genome_tools (the hints' plain ``open``) and
magot_smallfuncs (``ensure_file``, which tab2fasta reads through) get a shadow
that opens with ``newline='\\n'`` (lines end at LF only, nothing is translated)
and ``encoding='latin-1'`` (one character per byte), exactly as
make_golden_fasta.py's.

Per case: ``text`` (bytes as latin-1), ``fasta_out`` and ``fasta_exc`` of
tab2fasta on the file, ``literal_out`` and ``literal_exc`` of tab2fasta on the
text itself where it names no file, ``hints_out`` and ``hints_exc`` of the
hints, and ``fasta_path`` ('native', or why tab2fasta's device path is not
taken).  ``absent`` records the hints' exception for a path that does not open.

Usage:  python tests/golden/make_golden_tabcut.py
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
import tabcut_expect as te  # noqa: E402


def shadow(*modules):
    for m in modules:
        m.open = lambda path, *a, **k: builtins.open(path, newline='\n', encoding='latin-1')


def main():
    make_golden.reference_module()
    import genome_tools as tools
    import magot_smallfuncs as small
    shadow(tools, small)
    gold = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'table.tab')
        for name, text in te.cases().items():
            with open(path, 'wb') as fh:
                fh.write(text)
            _, fasta_exc, fasta_out = make_golden.call(lambda: tools.tab2fasta(path))
            _, hints_exc, hints_out = make_golden.call(
                lambda: tools.repeatmasker2augustushints(path))
            literal = text.decode('latin-1')
            literal_out = literal_exc = None
            if literal and len(literal) < 200 and not os.path.exists(literal):
                _, literal_exc, literal_out = make_golden.call(lambda: tools.tab2fasta(literal))
            gold[name] = {'text': literal, 'fasta_out': fasta_out, 'fasta_exc': fasta_exc,
                          'literal_out': literal_out, 'literal_exc': literal_exc,
                          'hints_out': hints_out, 'hints_exc': hints_exc,
                          'fasta_path': te.tab2fasta_path(text)}
            print(name, fasta_exc, hints_exc, len(fasta_out), len(hints_out), flush=True)
        _, absent_exc, absent_out = make_golden.call(
            lambda: tools.repeatmasker2augustushints(os.path.join(tmp, 'absent.gff')))
        assert absent_out == ''
    with open(os.path.join(HERE, 'tabcut.json'), 'w') as fh:
        json.dump({'cases': gold, 'absent': absent_exc}, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
