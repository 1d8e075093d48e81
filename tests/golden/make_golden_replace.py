"""Record what the REFERENCE's own replace_names prints: tests/golden/replace.json.

Runs only where the reference is installed (see make_golden.py, whose lib2to3
copy this imports); the reference function (genome_tools.py:431-446) runs
unchanged, and nothing of its program text is stored: only inputs, stdout,
exception names and each case's notes of its path.

The copy runs under Python 3, which differs from the Python 2 target in two
places this function touches; both are handled here, not in the copy.

  * ``open``: text mode would translate line ends and decode UTF-8.  The copied
    genome_tools gets a shadow that opens with ``newline='\\n'`` (lines end at LF
    only, nothing is translated) and ``encoding='latin-1'`` (one character per
    byte).
  * dict iteration order: every line sees the keys in the order of the dict.
    ``out`` is the reference's stdout as it came (first-seen order, the
    'insertion' record).  ``out_py2`` is a second run of the reference on the
    same table with its rows regrouped so that first-seen order equals the order
    a Python 2 dict of the keys ``name + name_end`` iterates
    (oracle.magot_oracle.py2_dict_order); all rows of one key stay together in
    their original order, which keeps first place and last value.  A last row
    without LF gets a TAB and an LF for that run (the same name and f1).  A
    table with a line without a TAB raises in both runs and is not regrouped.

Per case: ``text``, ``table`` and ``name_end`` (bytes as latin-1), ``out``,
``out_py2``, ``exc``, and ``path`` (per order: 'native', or why the device path
is not taken).

Usage:  python tests/golden/make_golden_replace.py
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
import replace_expect as rx  # noqa: E402
from oracle import magot_oracle as mo  # noqa: E402


def regrouped(table, name_end):
    """the table's rows grouped by key in Python 2's order of the keys"""
    try:
        rows = rx.table_rows(table)
    except IndexError:
        return table
    lines = rx.lines_of(table)
    if lines and not lines[-1].endswith(b'\n'):
        # the last row without LF may move up: a TAB and an LF behind it leave
        # its name and its f1 as they are
        lines[-1] += b'\t\n'
        assert rx.table_rows(b''.join(lines)) == rows
    keys = []
    for name, _ in rows:
        if name not in keys:
            keys.append(name)
    order = mo.py2_dict_order([(k + name_end).decode('latin-1') for k in keys])
    out = []
    for key in order:
        out += [line for line, (name, _) in zip(lines, rows)
                if (name + name_end).decode('latin-1') == key]
    return b''.join(out)


def main():
    make_golden.reference_module()
    import genome_tools as tools
    tools.open = lambda path, *a, **k: builtins.open(path, newline='\n', encoding='latin-1')
    gold = {}
    with tempfile.TemporaryDirectory() as tmp:
        path, table_path = os.path.join(tmp, 'text.txt'), os.path.join(tmp, 'names.tsv')
        for name, case in rx.cases().items():
            end = case['name_end'].decode('latin-1')
            with open(path, 'wb') as fh:
                fh.write(case['text'])
            outs = []
            for table in (case['table'], regrouped(case['table'], case['name_end'])):
                with open(table_path, 'wb') as fh:
                    fh.write(table)
                _, exc, out = make_golden.call(lambda: tools.replace_names(path, table_path, end))
                outs.append((out, exc))
            assert outs[0][1] == outs[1][1], name
            gold[name] = {'text': case['text'].decode('latin-1'),
                          'table': case['table'].decode('latin-1'), 'name_end': end,
                          'out': outs[0][0], 'out_py2': outs[1][0], 'exc': outs[0][1],
                          'path': rx.notes(case)}
            print(name, outs[0][1], gold[name]['path'], len(outs[0][0]), flush=True)
    with open(os.path.join(HERE, 'replace.json'), 'w') as fh:
        json.dump(gold, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
