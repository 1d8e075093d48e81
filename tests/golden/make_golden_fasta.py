"""Record what the REFERENCE's own exclude_from_fasta and fasta2tab print:
tests/golden/fasta.json.

Runs only where the reference is installed (see make_golden.py, whose lib2to3
copy this imports); both reference functions (genome_tools.py:377-391 and
:349-350 over magot_smallfuncs.py:21-29) run unchanged, and nothing of their
program text is stored: only inputs, stdout, exception names and each case's
note of its path.

The copy runs under Python 3, which differs from the Python 2 target in two
places these functions touch; both are handled here, not in the copy.

  * ``open``: text mode would translate line ends and decode UTF-8.  Every
    copied module that opens a file -- genome_tools (the exclusion list),
    magot_smallfuncs (``ensure_file``, which genome.GenomeSequence and fasta2tab
    read through) and genome -- gets a shadow that opens with ``newline='\\n'``
    (lines end at LF only, nothing is translated) and ``encoding='latin-1'``
    (one character per byte).
  * dict iteration order: the records are printed in the order of the
    sequence dict.  ``out`` is the reference's stdout as it came (first-seen
    order, the 'insertion' record).  ``out_py2`` holds the same records in the
    order a Python 2 dict of the keys iterates
    (oracle.magot_oracle.py2_dict_order): the generator knows the keys from its
    own input, takes each key's printed record from a second run of the
    reference that excludes nothing, and leaves out the keys the case's list
    names.  For a run that raises (a key without a word under
    just_firstword) it is cut before the first wordless key in that order.

No case holds a byte that Python 3's ``str.split`` takes for a blank and Python
2's does not (0x1c-0x1f, 0x85, 0xa0).

Per case: ``fasta`` and ``list`` (bytes as latin-1), ``kind`` ('file' or
'literal'), ``first_word``, ``out``, ``out_py2``, ``exc``, ``tab_out``,
``tab_exc``, and ``path``, ``tab_path`` ('native', or why the device path is
not taken).

Usage:  python tests/golden/make_golden_fasta.py
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
import fasta_expect as fe  # noqa: E402
from oracle import magot_oracle as mo  # noqa: E402

NOTHING = 'a name no record has'


def shadow(*modules):
    for m in modules:
        m.open = lambda path, *a, **k: builtins.open(path, newline='\n', encoding='latin-1')


def py2_record(case, blocks):
    """``out_py2`` from each key's printed record"""
    names = fe.exclusion_names(case['kind'], case['list'])
    out = []
    for key in mo.py2_dict_order([k.decode('latin-1') for k in fe.sequence_dict(case['fasta'])]):
        compared = key.encode('latin-1')
        if case['first_word']:
            words = compared.split()
            if not words:
                break
            compared = words[0]
        if compared not in names:
            out.append(blocks[key])
    return ''.join(out)


def printed_records(text):
    """'>key LF sequence LF' of every key, from a run that excludes nothing"""
    rows = text.split('\n')
    assert rows[-1] == '' and len(rows) % 2 == 1
    return {rows[i][1:]: rows[i] + '\n' + rows[i + 1] + '\n' for i in range(0, len(rows) - 1, 2)}


def main():
    make_golden.reference_module()
    import genome as ref_genome
    import genome_tools as tools
    import magot_smallfuncs as small
    shadow(tools, ref_genome, small)
    gold = {}
    with tempfile.TemporaryDirectory() as tmp:
        path, list_path = os.path.join(tmp, 'records.fa'), os.path.join(tmp, 'names.txt')
        for name, case in fe.cases().items():
            with open(path, 'wb') as fh:
                fh.write(case['fasta'])
            if case['kind'] == 'file':
                with open(list_path, 'wb') as fh:
                    fh.write(case['list'])
                arg = list_path
            else:
                arg = case['list'].decode('latin-1')
                assert not os.path.exists(arg)
            flag = 'True' if case['first_word'] else 'False'
            _, exc, out = make_golden.call(lambda: tools.exclude_from_fasta(path, arg, flag))
            _, all_exc, everything = make_golden.call(
                lambda: tools.exclude_from_fasta(path, NOTHING))
            assert all_exc is None
            _, tab_exc, tab_out = make_golden.call(lambda: tools.fasta2tab(path))
            note, tab_note = fe.notes(case)
            gold[name] = {'fasta': case['fasta'].decode('latin-1'), 'kind': case['kind'],
                          'list': case['list'].decode('latin-1'), 'first_word': case['first_word'],
                          'out': out, 'out_py2': py2_record(case, printed_records(everything)),
                          'exc': exc, 'tab_out': tab_out, 'tab_exc': tab_exc,
                          'path': note, 'tab_path': tab_note}
            print(name, exc, tab_exc, note, tab_note, len(out), flush=True)
    with open(os.path.join(HERE, 'fasta.json'), 'w') as fh:
        json.dump(gold, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
