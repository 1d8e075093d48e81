"""Record what the REFERENCE's own besthits_from_psl prints:
tests/golden/psl.json.

Runs only where the reference is installed (see make_golden.py, whose
lib2to3 copy this imports); the reference function (genome_tools.py:572-592)
runs unchanged, and nothing of its program text is stored: only inputs, stdout,
exception names and the case's note of its path.

The copy runs under Python 3, which differs from the Python 2 target in three
places this function touches; all are handled here, not in the copy.  Two names
are substituted in the copied module:

  * ``open``: text mode would translate line ends and decode UTF-8.  The shadow
    opens with ``newline='\\n'`` (lines end at LF only, nothing is translated)
    and ``encoding='latin-1'`` (one character per byte), as
    make_golden_overlap.py does.
  * ``int``: Python 3 reads ``1_0`` as 10 and digits beyond ASCII; Python 2
    rejects both.  The shadow is the Python 2 reading (psl_expect.py2_int:
    surrounding whitespace, one optional sign, ASCII digits).

And dict iteration order: the winners are printed in the order of the score
dict.  ``out`` is the reference's stdout as it came (first-seen order, the
'insertion' record).  ``out_py2`` is the same stdout with its last k lines --
the winners, k being the case's count of distinct keys, which this generator
knows from its own input -- put into the order a Python 2 dict of the
first-seen keys iterates (oracle.magot_oracle.py2_dict_order).  A case in which
the reference stops at an error line prints no winners and has one record:
``out_py2`` is null.  Whether it stops is read from the input here (a data
line with fewer than 10 fields, or an integer Python 2 rejects), not from the
output.

Per case: ``text`` (the file's bytes as latin-1), ``out``, ``out_py2``, ``exc``
(exception name or null) and ``path`` ('native', or why the device path must
decline).

Usage:  python tests/golden/make_golden_psl.py
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
import psl_expect as pe  # noqa: E402
from oracle import magot_oracle as mo  # noqa: E402


def shadow(tools):
    tools.open = lambda path, *a, **k: builtins.open(path, newline='\n', encoding='latin-1')
    tools.int = lambda s: pe.py2_int(s.encode('latin-1'))


def data_lines(text):
    return [ln.split(b'\t') for ln in pe.lines_of(text) if ln[:1] not in pe.PASS_BYTES]


def stops(text):
    """The reference meets a line it prints whole and returns at"""
    for fields in data_lines(text):
        try:
            fields[9], pe.py2_int(fields[0]), pe.py2_int(fields[1])
        except (IndexError, ValueError):
            return True
    return False


def py2_record(text, out):
    keys = []
    for fields in data_lines(text):
        key = fields[9].decode('latin-1')
        if key not in keys:
            keys.append(key)
    if not keys:
        return out
    lines = out.split('\n')
    assert lines[-1] == '' and len(lines) > len(keys)
    head, winners = lines[:-1 - len(keys)], lines[-1 - len(keys):-1]
    line_of = dict(zip(keys, winners))
    return '\n'.join(head + [line_of[k] for k in mo.py2_dict_order(keys)] + [''])


def main():
    make_golden.reference_module()
    import genome_tools as tools
    shadow(tools)
    gold = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'hits.psl')
        for name, (text, note) in pe.cases().items():
            with open(path, 'wb') as fh:
                fh.write(text)
            _, exc, out = make_golden.call(lambda: tools.besthits_from_psl(path))
            gold[name] = {'text': text.decode('latin-1'), 'out': out,
                          'out_py2': None if stops(text) else py2_record(text, out),
                          'exc': exc, 'path': note}
            print(name, exc, note, len(out), flush=True)
    with open(os.path.join(HERE, 'psl.json'), 'w') as fh:
        json.dump(gold, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
